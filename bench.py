#!/usr/bin/env python3
"""bench.py -- clips/sec of the M3T A+V hot path (forward + loss + backward [+ gradient
all-reduce + clip]) on synthetic 300-frame clips, BASELINE.json's metric.

Workload: feature-level audiovisual/attention graph --
audio GRU(128,256,2) | gru_v,gru_a GRU(256,512,2) | proj_v 2048->512 | AttFusion([512,512],128) |
fusion GRU(512,512,2,9,2) -- with the ccc_mtl training loss, 32 clips x 300 frames per GPU, fp32.
One process per GPU (torchrun), clips sharded across ranks (weak scaling), one flat-buffer RCCL
all-reduce of the gradients per step.

    python bench.py --gpus 1 --steps 10 --warmup 3
    python bench.py --gpus 1 --steps 10 --warmup 3 --full   # + CPU baseline, secondary configs, idle-queue enqueue probe
    python bench.py --gpus 8                      # starts its own 8 ranks (torch.distributed.run) before touching a GPU
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W [--scaling strong]

A plain run does what `value` and `ms_per_step` need: set-up, warm-up, the timed steps, --dump-outputs, the JSON line (with the
roofline and kernel figures read from HIP events of the timed steps themselves).  Everything that takes runs of its own -- the
CPU baseline, the secondary configurations (`aux`), the idle-queue enqueue probe (`host_enqueue_ms_idle`) and, for N > 1, the
back-to-back all-reduce -- runs only under --full; in a plain run their keys read null (`aux`, `aux_ms`, `speedup_vs_cpu`: absent).

Process structure for N > 1.  The process torchrun starts for a rank is a SUPERVISOR: it never touches the GPU, starts the
real worker (`--worker`) as a child and watches it.  If a worker reports a persistent scan that gave up (M3T_ESPIN: e.g. an
RCCL kernel and a resident-grid scan starving each other -- a combination no 1-GPU box can execute) or stops making
progress, every supervisor ends its worker and starts a fresh one on the launch-per-step scans with the gradient buckets
overlapped with backward; the JSON line then carries a "fallback" note.  N = 1 runs in the process itself, as before.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, "m3f.pytorch_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np
import torch
import torch.distributed as dist

FP32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_* = vector fp32 rate
HBM_PEAK_GBS = 8000.0


def synth_batch(B, T, d_a, d_v, device, rank):
    """np.random.RandomState(12345) (the reference's default --seed, train.py:49); each rank draws its own shard."""
    rs = np.random.RandomState(12345 + rank)
    f = lambda a: torch.from_numpy(a).to(device)
    return dict(
        x_v=f(rs.standard_normal((B, T, d_v)).astype(np.float32)),
        x_a=f(rs.standard_normal((B, T, d_a)).astype(np.float32)),
        valence=f(rs.uniform(-1, 1, (B, T)).astype(np.float32)),
        arousal=f(rs.uniform(-1, 1, (B, T)).astype(np.float32)),
        class_expr=f(rs.randint(0, 7, (B, T)).astype(np.int64)),
        expr_valid=f(rs.uniform(size=(B, T)) < 0.7),
    )


def usable_cores():
    """Host cores this process may actually use: affinity mask, capped by the cgroup CPU quota."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = max(1, min(n, int(float(quota) / float(period) + 0.5)))
    except Exception:  # noqa: BLE001
        pass
    return n


def cpu_baseline(max_clips, T, d_a, d_v, budget_s=25.0):
    """The same workload from stock torch CPU ops (== the reference's CPU path, oracle/torch_ref.py),
    timed on this box's host cores on a bounded sample: max_clips clips per iteration, one warm-up and
    2..6 timed iterations within the budget."""
    from oracle import torch_ref as R
    cores = usable_cores()
    torch.set_num_threads(cores)
    torch.manual_seed(12345)
    m = R.RefAVFeatureGraph(d_a, d_v, 512)
    full = synth_batch(max_clips, T, d_a, d_v, "cpu", 0)

    def it(nb):
        for p in m.parameters():
            p.grad = None
        y = m(full["x_a"][:nb], full["x_v"][:nb])
        R.mtl_loss(y, full["valence"][:nb], full["arousal"][:nb], full["class_expr"][:nb], full["expr_valid"][:nb]).backward()

    t_all = time.perf_counter()
    nb = max_clips                          # batch-1 recurrences are GEMV-bound on CPU: time a real mini-batch
    it(nb)                                  # warm-up
    n, t0 = 0, time.perf_counter()
    while n < 2 or (n < 6 and time.perf_counter() - t_all < budget_s):
        it(nb)
        n += 1
    dt = (time.perf_counter() - t0) / n
    return {"value": round(nb / dt, 3), "unit": "clips/s", "cores": cores, "kind": "port",
            "sample": "%d iterations of fwd+loss+bwd on %d clips x %d frames (stock torch CPU ops = the reference's "
                      "CPU path, fp32, %d threads of os.cpu_count()=%d, %.2f s/iter)"
                      % (n, nb, T, cores, os.cpu_count() or 0, dt)}


# ---- secondary configurations of BASELINE.json (configs[0], [1], [4]): timed OUTSIDE `value`, reported under "aux" ----------
# algorithmic FLOPs per clip, forward + backward = 3 x forward: C1 TCN head 128 -> 512 -> 512, k=3 + Linear(512, 2)
# at T=300: 3 x 1.573 GF; C2 TCN(256 -> 512 -> 512) -> GRU(512,512,2,2,2) at T=300: 20.29 GF; C5 full AffWild2VA A+V on 112x112
# frames at T=64: 135 GF.
AUX_FLOPS = {"c1": 3 * 1.573e9, "c2": 20.29e9, "c2bf16": 20.29e9, "c5": 135e9, "c3high": 47.43e9, "c3x6": 47.43e9, "c3fp32": 47.43e9,
             "c3_eval": 47.43e9 / 3, "c5_eval": 135e9 / 3}      # (forward only: a third of forward + backward)      # (c3high: the main workload, 47.43 GF per clip)


def aux_child(which, steps=10, warmup=3):
    """runs in a child process of bench.py (`--aux-child`): one JSON line per finished configuration"""
    from m3t import ops
    from m3t.workloads import TcnHead, TcnGru, make_seq_step
    from m3t.ddp import FlatGradDDP
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)

    def timed(step, steps=steps):
        import gc
        steps = int(os.environ.get("M3T_AUX_STEPS", steps))
        for _ in range(warmup):
            step()
        torch.cuda.synchronize()
        gc.collect()                      # as the main leg: no generation-2 collector pause inside the few timed steps ...
        gc.freeze()                       # ... and the survivors of the earlier legs (models, cached workspaces, ctypes tables) out of the
                                          # collector's sight: the C5 leg, run behind five others in one process, was 1.5 ms slower than alone
                                          # (host-side: until the count of valid labels travelled ahead of the forward pass, its launches were enqueued between two syncs)
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        th = time.perf_counter() - t0
        torch.cuda.synchronize()
        ops.poll_scan_error()
        if os.environ.get("M3T_BENCH_STEP_TIMES") == "1":
            print("# aux host enqueue %.3f ms per step" % (th / steps * 1e3), file=sys.stderr, flush=True)
        return (time.perf_counter() - t0) / steps * 1e3

    def emit(key, workload, clips, ms, dtype):
        print(json.dumps({"aux": key, "workload": workload, "clips": clips, "ms_per_step": round(ms, 3),
                          "clips_per_s": round(clips / ms * 1e3, 1), "dtype": dtype,
                          "alg_tflops": round(AUX_FLOPS[key] * clips / ms / 1e9, 2)}), flush=True)

    rs = np.random.RandomState(12345)
    f = lambda a: torch.from_numpy(a).to(dev)
    B, T = 32, 300
    val, aro = f(rs.uniform(-1, 1, (B, T)).astype(np.float32)), f(rs.uniform(-1, 1, (B, T)).astype(np.float32))
    if "c1" in which:
        torch.manual_seed(12345)
        m = TcnHead(128, 512, 2).to(dev).train()
        x = f(rs.standard_normal((B, 128, T)).astype(np.float32))
        _, step = make_seq_step(m, x, val, aro)
        emit("c1", "C1 TemporalConvNet(128,[512,512],3)+Linear(512,2), train mode (dropout 0.2), ccc loss, fwd+bwd+clip, 32x300", B, timed(step, 30), "f32")
    if "c2" in which or "c2bf16" in which:
        torch.manual_seed(12345)
        m = TcnGru(256, 512).to(dev).train()
        x = f(rs.standard_normal((B, 256, T)).astype(np.float32))
        _, step = make_seq_step(m, x, val, aro)
        if "c2" in which:
            emit("c2", "C2 TemporalConvNet(256,[512,512],3)->GRU(512,512,2,2,2), train mode, ccc loss, fwd+bwd+clip, 32x300, fp32", B, timed(step, 30), "f32")
        if "c2bf16" in which:
            def step16():
                with ops.precision("bf16"):
                    step()
            emit("c2bf16", "C2 as above with bf16 matmul/conv/recurrent operands, fp32 accumulate/state/master weights (BASELINE configs[1])", B,
                 timed(step16, 30), "bf16 operands, f32 accumulate")
    if "c3x6" in which:
        # the MAIN workload with the round-2 arithmetic -- every GEMM / conv / recurrent product from three bf16 terms and six MFMAs
        # (ops.precision("x6")) -- on the same box in the same run: what the default's two-fp16-term products (DESIGN.md section 7 / NOTEBOOK.md section 5e)
        # are worth.  Both modes are fp32-accurate; `value` is the default's.
        from m3t.workloads import AVFeatureGraph, make_c3_step
        torch.manual_seed(12345)
        m6 = AVFeatureGraph(128, 256, 512).to(dev)
        _, step6 = make_c3_step(m6, synth_batch(B, T, 128, 256, dev, 0), max_norm=1.0)

        def step_x6():
            with ops.precision("x6"):
                step6()
        emit("c3x6", "C3/C4 main workload with ops.precision('x6'): every fp32-accurate product from three bf16 terms and six MFMAs (the "
             "default until round 3) instead of two fp16 terms of the scaled operands and three", B, timed(step_x6, 30), "f32 (bf16x6 products)")
        del m6, step6
    if "c3fp32" in which:
        # the MAIN workload on EXACT fp32 arithmetic: this child runs with M3T_GEMM_X6=0 and M3T_SCAN_X6=0 (run_aux sets them), i.e. every GEMM
        # and every recurrent product on v_mfma_f32_*_f32 (fp32 operands, 157 TFLOP/s peak) -- beside the emulated-fp32 headline (two fp16
        # terms, three MFMAs) and the strict six-product mode (aux.c3x6) on the same box in the same run
        from m3t.workloads import AVFeatureGraph, make_c3_step
        torch.manual_seed(12345)
        m32 = AVFeatureGraph(128, 256, 512).to(dev)
        _, step32 = make_c3_step(m32, synth_batch(B, T, 128, 256, dev, 0), max_norm=1.0)
        emit("c3fp32", "C3/C4 main workload with every GEMM and recurrent product on fp32-input MFMAs (M3T_GEMM_X6=0, M3T_SCAN_X6=0): exact fp32 "
             "operands, no emulation", B, timed(lambda: step32(), 20), "f32 (fp32-input MFMA)")
        del m32, step32
    if "c3_eval" in which:
        # inference: the forward pass of validation_step / test_step (reference models/model.py:226-246,320-337: self.forward(batch) on
        # windows, eval mode, no autograd graph) on the main workload's batch
        from m3t.workloads import AVFeatureGraph
        torch.manual_seed(12345)
        me = AVFeatureGraph(128, 256, 512).to(dev).eval()
        be = synth_batch(B, T, 128, 256, dev, 0)

        def fwd_e():
            with torch.no_grad():
                me(be["x_a"], be["x_v"])
        emit("c3_eval", "C3/C4 graph, forward only under torch.no_grad(), eval mode (validation_step / test_step), 32x300", B, timed(fwd_e, 30), "f32")
        del me
    if "c3high" in which:
        # the MAIN workload in the opt-in "high" matmul precision (two bf16 terms per GEMM / conv operand, four products: what
        # torch.set_float32_matmul_precision('high') means; recurrent scans unchanged) -- NOT the headline: `value` is measured
        # in the default fp32-accurate mode.  Accuracy of the mode: tests/test_gpu_high.py (y within 5e-6 of the reference golden)
        from m3t.workloads import AVFeatureGraph, make_c3_step
        torch.manual_seed(12345)
        m = AVFeatureGraph(128, 256, 512).to(dev)
        _, step3 = make_c3_step(m, synth_batch(B, T, 128, 256, dev, 0), max_norm=1.0)

        def step_high():
            with ops.precision("high"):
                step3()
        emit("c3high", "C3/C4 main workload with ops.precision('high'): GEMM operands as two bf16 terms (4 products, ~2^-16 per term), "
             "scans fp32-accurate; opt-in mode, not the headline", B, timed(step_high, 30), "f32 operands as 2 x bf16 in GEMMs, f32 accumulate")
    if "cbam" in which:
        # the HBM-bound kernel family of the path: models.cbam.CBAM forward + backward on the four
        # ResNet-18 stage shapes of a 32 x 64-frame batch (2048 frames), bytes / time against the 8 TB/s HBM roofline.
        # Algorithmic passes over a tensor of x's size, forward + backward, with BatchNorm2d(1) in train mode (two global
        # statistics -- one forward, one backward -- each cut the gate in two): fwd read x | read x, write y; bwd read dy,
        # read x | read dy, read x, write dx = 8; `GBps_8pass` = 8 x bytes(x) / time.
        from models.cbam import CBAM
        res = {}
        for (Cc, HWs) in ((64, 28), (128, 14), (256, 7), (512, 4)):
            torch.manual_seed(0)
            cb = CBAM(Cc).to(dev).train()
            xx = torch.randn(2048, Cc, HWs, HWs, device=dev, requires_grad=True)
            gg = torch.randn(2048, Cc, HWs, HWs, device=dev)

            cb_params = list(cb.parameters())       # (walking the module tree costs 40 us per call: as long as the 4 x 4 stage's F1)

            def fb():
                for p_ in cb_params:
                    p_.grad = None
                xx.grad = None
                cb(xx).backward(gg)
            ms = timed(fb, 20)
            # the same 20 iterations with the host taken out of the measurement: the GPU is parked behind a 30 ms spin kernel while
            # the host enqueues all of them, HIP events bracket their execution.  At the late stages the gate's kernels take ~0.2 ms
            # and one forward + backward through autograd costs the host about as much (tools/cbam_host.py), so the wall figure
            # above is the enqueue path's as much as the kernels'; ms_fwd_bwd stays the wall figure.
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            torch.cuda._sleep(int(0.03 * 2.4e9))
            e0.record()
            for _ in range(20):
                fb()
            e1.record()
            torch.cuda.synchronize()
            gms = e0.elapsed_time(e1) / 20
            nbytes = xx.numel() * 4
            res["%dx%dx%d" % (Cc, HWs, HWs)] = {"frames": 2048, "x_bytes": nbytes, "ms_fwd_bwd": round(ms, 4),
                                                "GBps_8pass": round(8 * nbytes / ms / 1e6, 1),
                                                "frac_of_hbm_peak": round(8 * nbytes / ms / 1e6 / HBM_PEAK_GBS, 4),
                                                "gpu_ms_fwd_bwd": round(gms, 4),
                                                "gpu_frac_of_hbm_peak": round(8 * nbytes / gms / 1e6 / HBM_PEAK_GBS, 4)}
            del xx, gg, cb
        print(json.dumps({"aux": "cbam", "workload": "models.cbam.CBAM forward + backward (train mode: BatchNorm2d(1) batch statistics) on the four ResNet-18 stage "
                          "shapes, 2048 frames each; GBps_8pass = 8 x bytes(x) / time, the fused operator's algorithmic HBM passes (DESIGN.md section 4)",
                          "stages": res, "dtype": "f32", "peak_GBps": HBM_PEAK_GBS}), flush=True)
    if "c5" in which:
        if os.environ.get("M3T_AUX_EMPTY_CACHE", "1") != "0":
            import gc
            gc.collect()
            torch.cuda.empty_cache()      # the earlier legs' cached blocks (other shapes) back to the driver: this leg allocates 6 GB of its own
        from models.model import AffWild2VA
        hp = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
        hp.modality, hp.fusion_type, hp.loss, hp.window = "audiovisual", "attention", "ccc_mtl", 64
        Bc, Tc = 8, 64
        torch.manual_seed(12345)
        m = AffWild2VA(hp).to(dev).train()
        batch = {"video": f(rs.randint(0, 256, (Bc, 3, Tc, 112, 112)).astype(np.float32)), "se_features": f(rs.standard_normal((Bc, 512, Tc)).astype(np.float32)),
                 "audio": f(rs.standard_normal((Bc, Tc, 200)).astype(np.float32)),
                 "label_valence": f(rs.uniform(-1, 1, (Bc, Tc)).astype(np.float32)), "label_arousal": f(rs.uniform(-1, 1, (Bc, Tc)).astype(np.float32)),
                 "class_expr": f(rs.randint(0, 7, (Bc, Tc)).astype(np.int64)), "expr_valid": f(rs.uniform(size=(Bc, Tc)) < 0.7)}
        ddp = FlatGradDDP(m, max_norm=1.0)

        def step5():
            ddp.zero_grad()
            m.training_step(batch, 0)["loss"].backward()
            ddp.finish()
        ms5 = timed(step5)      # (training_step decides on the expression branch from a count queued BEFORE the forward pass: no stall after the loss;
                                # M3T_STEP_SYNC=1 reads the statistics back after the loss as the reference's two .item() calls do)
        # the enqueue path of the two halves of the step with the GPU parked behind a spin kernel (no back-pressure; the count of valid labels
        # is left out: reading it would wait for the spin): forward + loss, then backward + clip, and the GPU's time for each half once
        # the whole half is queued ahead (HIP events behind the spin)
        halves = []
        for _ in range(3):
            ddp.zero_grad()
            torch.cuda.synchronize()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            torch.cuda._sleep(int(0.03 * 2.4e9)); ev[0].record(); t0 = time.perf_counter()
            loss5 = m.va_objective(m.forward(batch), batch)[0]
            t1 = time.perf_counter(); ev[1].record(); torch.cuda.synchronize()
            torch.cuda._sleep(int(0.03 * 2.4e9)); ev[2].record(); t2 = time.perf_counter()
            loss5.backward(); ddp.finish()
            t3 = time.perf_counter(); ev[3].record(); torch.cuda.synchronize()
            halves.append(((t1 - t0) * 1e3, (t3 - t2) * 1e3, ev[0].elapsed_time(ev[1]), ev[2].elapsed_time(ev[3])))
            del loss5
        hv = [round(sorted(h[i] for h in halves)[1], 3) for i in range(4)]
        print(json.dumps({"aux": "c5_halves", "host_enqueue_ms_idle": round(hv[0] + hv[1], 3), "host_forward_loss_ms": hv[0], "host_backward_clip_ms": hv[1],
                          "gpu_forward_loss_ms": hv[2], "gpu_backward_clip_ms": hv[3],
                          "note": "median of 3; GPU parked behind a 30 ms spin kernel while the host enqueues each half of the C5 step; gpu_* = HIP events "
                                  "around the half once it is all queued"}), flush=True)
        print(json.dumps({"aux": "c5", "workload": "C5 AffWild2VA(audiovisual, attention, v2p_split, ccc_mtl) on raw 112x112 frames: the VGG-M stems as a channels-last chain (round 6: tap-walk convolutions reading and writing [N T H W][C] rows, BatchNorm3d+ReLU and MaxPool3d on the same rows, no transposes, fp16x3), training_step+bwd+clip, 8x64",
                          "clips": Bc, "ms_per_step": round(ms5, 3), "clips_per_s": round(Bc / ms5 * 1e3, 1), "dtype": "f32",
                          "alg_tflops": round(AUX_FLOPS["c5"] * Bc / ms5 / 1e9, 2)}), flush=True)
        if "c5_eval" in which:
            m.eval()

            def fwd5():
                with torch.no_grad():
                    m(batch)
            emit("c5_eval", "C5 AffWild2VA forward only under torch.no_grad(), eval mode (validation_step / test_step windows of 64 frames): the "
                 "stems' convolutions on the same tap walks as training (one path whatever the grad mode)", Bc, timed(fwd5), "f32")
            from m3t import ops as _o
            print(json.dumps({"aux": "stock_fallbacks", "calls_by_site": dict(_o.STOCK_FALLBACKS), "conv_forward_calls_by_path": dict(_o.CONV3D_CALLS)}), flush=True)


    if "cbam" in which or "resnet3d" in which:          # ("resnet3d": this step without the four gate shapes above -- profiling runs)
        if os.environ.get("M3T_AUX_EMPTY_CACHE", "1") != "0":
            import gc
            gc.collect()
            torch.cuda.empty_cache()
        # inside a model: VA_3DResNet(resnet_ver='v1', use_cbam=True) visual-only, 8 clips x 64 frames of 112 x 112 (SURVEY 8(d) C5 alt)
        from models.backbone import VA_3DResNet
        Bc, Tc = 8, 64
        torch.manual_seed(12345)
        net = VA_3DResNet(inputDim=512, hiddenDim=512, nLayers=2, nClasses=2, frameLen=Tc, use_cbam=True, resnet_ver="v1").to(dev).train()
        vid = f(((rs.randint(0, 256, (Bc, 3, Tc, 112, 112)).astype(np.float32)) - 127.5) / 127.5)
        ddp = FlatGradDDP(net, max_norm=1.0)

        def step_r():
            ddp.zero_grad()
            y = net(vid)
            ops.va_loss(y, val[:Bc, :Tc].contiguous(), aro[:Bc, :Tc].contiguous())[0].backward()
            ddp.finish()
        ms = timed(step_r, 10)
        print(json.dumps({"aux": "cbam_resnet3d", "workload": "VA_3DResNet(resnet_ver='v1', use_cbam=True) visual-only training step (SURVEY 8(d) C5 alt), 8 clips x 64 "
                          "frames of 112 x 112: 3-D stem + per-frame ResNet-18 convolutions: forward, weight gradient and data gradient (the strided layers' as parity-class walks) as tap-walk implicit GEMMs over channels-last activations (fp16x3, no patch matrix, no MIOpen kernel); the 8 CBAM gates, BatchNorm and the BiGRU head on the HIP kernels",
                          "clips": Bc, "ms_per_step": round(ms, 3), "clips_per_s": round(Bc / ms * 1e3, 1), "dtype": "f32"}), flush=True)


def run_aux(which, budget_s):
    """the aux leg in a child process with a wall-clock budget (MIOpen's first-use kernel search for the C5 stem can take long
    on a fresh box): whatever finished in time is reported"""
    import subprocess
    env = dict(os.environ, M3T_SCAN_LOCK="0")          # this process owns the GPU's persistent-scan lock and is idle meanwhile
    names = [w for w in which.split(",") if w]
    res, note, out = {}, None, ""
    t_start = time.perf_counter()
    # (the exact-fp32 leg needs the library's environment switches: a child of its own, first -- it is short)
    legs = ([(["c3fp32"], dict(env, M3T_GEMM_X6="0", M3T_SCAN_X6="0"))] if "c3fp32" in names else []) + \
           [([w for w in names if w != "c3fp32"], env)]
    for leg, leg_env in legs:
        if not leg:
            continue
        left = budget_s - (time.perf_counter() - t_start)
        if left <= 5:
            note = "aux leg cut at its %d s budget" % budget_s
            break
        cmd = [sys.executable, os.path.abspath(__file__), "--aux-child", ",".join(leg)]
        try:
            p = subprocess.run(cmd, env=leg_env, capture_output=True, text=True, timeout=left)
            out += p.stdout
            if p.returncode != 0:
                note = "aux child exited with %d: %s" % (p.returncode, p.stderr[-300:])
        except subprocess.TimeoutExpired as e:
            out += e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or "")
            note = "aux leg cut at its %d s budget" % budget_s
    for line in out.splitlines():
        if line.startswith('{"aux"'):
            d = json.loads(line)
            res[d.pop("aux")] = d
    if note:
        res["note"] = note
    return res


ESPIN_EXIT = 42          # a worker that saw M3T_ESPIN exits with this code: its supervisor starts the fallback
STORE_PORT_OFFSET = 17   # supervisors' coordination store: MASTER_PORT + 17; workers rendezvous on MASTER_PORT + 1 + attempt


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=32, help="clips per GPU (weak scaling) / global batch (strong scaling)")
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="weak",
                    help="weak: --batch clips on EVERY GPU; strong: --batch clips in all, split over the GPUs (SURVEY 8(d) C4)")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements beyond the headline: CPU baseline, secondary configs (--aux), idle-queue enqueue probe, "
                         "back-to-back all-reduce (N > 1)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--cpu-clips", type=int, default=32, help="clips per CPU-baseline iteration (default: the GPU's batch)")
    ap.add_argument("--aux", default="c3fp32,c1,c2,c2bf16,c3x6,c3_eval,c5,c5_eval,cbam",
                    help="secondary configs timed after the main leg at N=1 under --full ('' = none)")
    ap.add_argument("--aux-budget", type=float, default=240.0)
    ap.add_argument("--aux-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--worker", type=int, default=None, help=argparse.SUPPRESS)      # attempt number (0, or 1 = fallback)
    ap.add_argument("--worker-timeout", type=float, default=float(os.environ.get("M3T_BENCH_WORKER_TIMEOUT", "900")),
                    help="N > 1: seconds a worker may go WITHOUT a heartbeat (one per step and phase) before its supervisor declares it stuck "
                         "and starts the fallback")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (rank 0) as DIR/<name>.npy: see dump_outputs()")
    return ap.parse_args()


DUMP_GRAD_SAMPLE = 1 << 22         # gradient values kept by --dump-outputs (16 MB of fp32; the whole flat gradient is ~106 MB)


def dump_outputs(out_dir, model, ddp, res):
    """--dump-outputs: what a caller of the timed step receives, from its last timed call, as float32 / float64 .npy files
    (about 17 MB in all).  y [B, T, 9] (the model's output), loss [1], stats [8] (ops.va_loss), grad_norm [1] (the norm the clip
    saw), grad_param_norms [one per parameter tensor] (fp64 L2 norm of every parameter's clipped gradient, named_parameters() order) and
    grad_sample: DUMP_GRAD_SAMPLE entries of the clipped gradients concatenated in that order, at sorted indices drawn by
    np.random.RandomState(0) -- the same indices in every run with the same arguments."""
    loss, stats, y = res
    os.makedirs(out_dir, exist_ok=True)
    grads = [(p.grad if p.grad is not None else torch.zeros_like(p)).detach().reshape(-1).cpu().numpy() for p in model.parameters()]
    flat = np.concatenate(grads).astype(np.float32, copy=False)
    k = min(flat.size, DUMP_GRAD_SAMPLE)
    idx = np.sort(np.random.RandomState(0).choice(flat.size, k, replace=False))
    arrays = {
        "y": y.detach().float().cpu().numpy(),
        "loss": loss.detach().double().reshape(1).cpu().numpy(),
        "stats": stats.detach().double().reshape(-1).cpu().numpy(),
        "grad_norm": torch.as_tensor(ddp.last_norm).detach().double().reshape(-1).cpu().numpy(),
        "grad_param_norms": np.array([np.linalg.norm(g.astype(np.float64)) for g in grads]),
        "grad_sample": flat[idx],
    }
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return {name: list(a.shape) for name, a in arrays.items()}


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(args):
    """`python bench.py --gpus N` with no WORLD_SIZE in the environment: start the N ranks ourselves, as the driver would.
    Nothing in THIS process has touched the GPU (importing torch does not initialise HIP), and it never will: it only
    waits for torch.distributed.run and passes its exit code on."""
    import subprocess
    port = int(os.environ.get("MASTER_PORT", _free_port()))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    print("# bench.py --gpus %d without a launcher: starting %s" % (args.gpus, " ".join(cmd[1:8])), file=sys.stderr, flush=True)
    return subprocess.call(cmd)


def supervise(args):
    """The process torchrun started for this rank (N > 1).  No GPU call here.  Runs the worker as a child; all supervisors share
    a TCPStore (rank 0 hosts it, CPU only) through which the first one that sees a failed or stuck worker calls the fallback."""
    import subprocess
    from datetime import timedelta
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    port = int(os.environ.get("MASTER_PORT", "29500"))
    store = dist.TCPStore("127.0.0.1", port + STORE_PORT_OFFSET, world, rank == 0, timedelta(seconds=300), wait_for_workers=False)
    me = [sys.executable, os.path.abspath(__file__)] + sys.argv[1:]

    def run(attempt, extra_env):
        import tempfile
        env = dict(os.environ, **extra_env)
        env.pop("TORCHELASTIC_USE_AGENT_STORE", None)        # the workers host their own rendezvous store (port + 1 + attempt)
        # heartbeat: the worker touches this file at every step and phase (the limit used to run from the worker's START, so a
        # healthy long run was killed -- and silently re-run in the fallback configuration -- while "no progress" was the claim)
        hb = tempfile.NamedTemporaryFile(prefix="m3t_bench_hb_%d_" % rank, delete=False)
        hb.close()
        env["M3T_BENCH_HEARTBEAT"] = hb.name
        p = subprocess.Popen(me + ["--worker", str(attempt)], env=env)
        key = "fail%d" % attempt

        def beat_age():
            try:
                return time.time() - os.stat(hb.name).st_mtime
            except OSError:
                return 0.0

        def done(rc_):
            try:
                os.unlink(hb.name)
            except OSError:
                pass
            return rc_

        while True:
            rc = p.poll()
            if rc is not None:
                if rc != 0:
                    store.set(key, "rank %d exited with %d" % (rank, rc))
                return done(rc)
            failed = store.check([key])
            if not failed and beat_age() > args.worker_timeout:
                store.set(key, "rank %d made no progress for %.0f s" % (rank, args.worker_timeout))
                failed = True
            if failed:
                # some rank's worker failed: ours is waiting in a collective for it (or is the stuck one) -- end exactly it
                p.kill()
                p.wait()
                return done(-1)
            time.sleep(0.25)

    def leave(rc):
        # rank 0 hosts the store: it may only go once every other supervisor has said goodbye
        store.add("bye", 1)
        while rank == 0 and int(store.add("bye", 0)) < world:
            time.sleep(0.1)
        return rc

    rc = run(0, {})
    store.add("done0", 1)
    while int(store.add("done0", 0)) < world:                # every supervisor has its first verdict (and its worker is gone)
        time.sleep(0.1)
    if not store.check(["fail0"]):
        return leave(rc)
    why = store.get("fail0").decode()
    if rank == 0:
        print("# worker failure (%s): fresh workers on the launch-per-step scans with overlapped gradient buckets" % why,
              file=sys.stderr, flush=True)
    rc = run(1, {"M3T_SCAN_PERSIST": "0", "M3T_BENCH_FALLBACK": why})
    store.add("done1", 1)
    while int(store.add("done1", 0)) < world:
        time.sleep(0.1)
    return leave(1 if store.check(["fail1"]) else rc)


def main():
    args = parse_args()
    if args.aux_child is not None:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
        aux_child(set(args.aux_child.split(",")))
        return
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args))                    # before anything touches the GPU
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    if world > 1 and args.worker is None:
        sys.exit(supervise(args))                      # likewise: the supervisor never touches the GPU
    try:
        worker(args)
    except Exception as e:  # noqa: BLE001
        if world > 1 and "M3T_ESPIN" in str(e):
            print("# rank %s: %s" % (os.environ.get("RANK"), e), file=sys.stderr, flush=True)
            sys.stderr.flush()
            os._exit(ESPIN_EXIT)                       # no teardown: peers may be waiting in a collective for this rank
        raise


def worker(args):
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    fallback = os.environ.get("M3T_BENCH_FALLBACK")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the hot path has no CPU fallback")
    # M3T_BENCH_BACKEND=gloo + M3T_BENCH_ONE_DEVICE=1 let the N>1 code path be exercised on a 1-GPU box
    # (all ranks on cuda:0, gloo all-reduce); the real multi-GPU run uses RCCL ("nccl"), one GPU per rank.
    backend = os.environ.get("M3T_BENCH_BACKEND", "nccl")
    dev_index = 0 if os.environ.get("M3T_BENCH_ONE_DEVICE") == "1" else local_rank
    if os.environ.get("M3T_BENCH_ONE_DEVICE") == "1" and world > 1:
        # several processes on ONE device: persistent scan launches of different processes could each hold part of the
        # chip while waiting for the rest of their grid -- take the launch-per-step scans (include/m3t_hip.h)
        os.environ["M3T_SCAN_PERSIST"] = "0"
    torch.cuda.set_device(dev_index)
    device = torch.device("cuda", dev_index)
    if world > 1:
        port = int(os.environ.get("MASTER_PORT", "29500")) + 1 + int(args.worker or 0)
        kw = dict(init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device, **kw)
        else:
            dist.init_process_group(backend, **kw)
        if dist.get_world_size() != args.gpus:
            raise SystemExit("--gpus %d but the process group has %d ranks" % (args.gpus, dist.get_world_size()))

    from m3t.workloads import AVFeatureGraph, make_c3_step
    from m3t import ops

    B, T, d_a, d_v = args.batch, args.frames, 128, 256
    if args.scaling == "strong":
        if args.batch % world:
            raise SystemExit("--scaling strong: --batch %d is not divisible by %d GPUs" % (args.batch, world))
        B = args.batch // world                    # the global batch is fixed, each GPU gets 1/N of it
    torch.manual_seed(12345)                       # identical replicas on every rank
    model = AVFeatureGraph(d_a, d_v, 512).to(device)
    n_params = sum(p.numel() for p in model.parameters())
    batch = synth_batch(B, T, d_a, d_v, device, rank)
    # the step (m3t/workloads.py): zero_grad -> forward -> ccc_mtl loss -> backward -> all-reduce (N > 1) + 1/N + clip 1.0.
    # tests/test_gpu_bench_path.py runs this same function at B=32 x T=300 against a reference-generated golden.
    ddp, step_fn = make_c3_step(model, batch, max_norm=1.0)
    last = [None]                                   # --dump-outputs: (loss, stats, y) of the latest step

    def step():
        res = step_fn()
        if args.dump_outputs:
            last[0] = res
        return res[0].detach()

    def fence():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    from m3t import _lib
    hb_path = os.environ.get("M3T_BENCH_HEARTBEAT")

    def beat():                                      # N > 1: tell the supervisor this worker is alive (its limit is on heartbeat AGE)
        if hb_path:
            try:
                os.utime(hb_path, None)
            except OSError:
                pass

    beat()
    for _ in range(args.warmup):
        step()
        beat()
    if os.environ.get("M3T_BENCH_INJECT_FAULT") == str(rank) and not (args.worker or 0):
        # fault injection (tests of the supervisors' fallback): this rank's first attempt sees "a persistent scan gave up"
        ops.inject_scan_error()
    fence()
    ops.PROFILE.clear()
    n_persist0 = _lib.load().m3t_gru_persist_count()
    # HIP events around the scan launches (roofline.achieved), on every EVENTS_EVERY-th step of the timed region: an event
    # pair per launch costs the step 0.8 ms (4 %) when every launch of every step carries one -- measured, M3T_BENCH_EVENTS=1
    events_every = max(1, int(os.environ.get("M3T_BENCH_EVENTS", "4")))
    timed_steps = 0
    ar_events = []
    step_marks = [] if os.environ.get("M3T_BENCH_STEP_TIMES") == "1" else None      # debugging: per-step GPU time on stderr
    host_marks = []
    # Python's cyclic collector: a generation-2 pass over the heap of this process (torch + numpy + distributed) stops the host
    # for 45-100 ms.  Landing in the first timed steps -- the GPU idle after the fence, the host with no lead yet -- it starved the
    # GPU for that long and put 0.5-2 ms on the mean of a 20-30 step run (per-step times: M3T_BENCH_STEP_TIMES=1).  Collect now and
    # move the survivors out of the collector's sight, as m3t.trainer.Trainer.fit does after its first step.
    if os.environ.get("M3T_BENCH_GC", "1") != "0":
        import gc
        gc.collect()
        gc.freeze()
    t0 = time.perf_counter()
    for i in range(args.steps):
        ops.PROFILE_ON[0] = i % events_every == 0
        timed_steps += int(ops.PROFILE_ON[0])
        if world > 1:
            # N > 1: an event pair around the in-step gradient all-reduce (poison kernel, collective, dead-rank check) on the
            # profiled steps: `allreduce.ms_in_step` is what the collective costs INSIDE the step, on the step's own stream
            ddp.ar_events = ar_events if ops.PROFILE_ON[0] else None
        loss = step()
        beat()
        if step_marks is not None:
            step_marks.append(torch.cuda.Event(enable_timing=True))
            step_marks[-1].record()
            host_marks.append(time.perf_counter())
    ops.PROFILE_ON[0] = False
    ddp.ar_events = None
    host_ms = (time.perf_counter() - t0) / args.steps * 1e3      # host time to ENQUEUE a step (no sync inside the loop)
    fence()
    dt = time.perf_counter() - t0
    if step_marks:
        print("# per-step ms: " + " ".join("%.2f" % a.elapsed_time(b) for a, b in zip(step_marks[:-1], step_marks[1:])),
              file=sys.stderr, flush=True)
        print("# host per-step ms: " + " ".join("%.2f" % ((b - a) * 1e3) for a, b in zip([t0] + host_marks[:-1], host_marks)),
              file=sys.stderr, flush=True)
    dumped = None
    if args.dump_outputs and rank == 0:             # outside the timed region, before the enqueue probe below runs more steps
        dumped = dump_outputs(args.dump_outputs, model, ddp, last[0])
    beat()
    persist_per_step = (_lib.load().m3t_gru_persist_count() - n_persist0) / max(1, args.steps)     # (the timed steps' launches only)
    # --full: host enqueue cost with an IDLE queue: the GPU is parked behind a spin kernel while the host enqueues whole
    # steps, so the figure has no queue back-pressure in it -- `host_enqueue_ms_per_step` above mixes the two (a host that runs ahead of the
    # GPU blocks in the driver's full queue and reads as "slow host").  Outside the timed region; 3 steps behind ~60 ms of spin.
    host_idle_ms = None
    if args.full and world == 1:
        try:
            torch.cuda.synchronize()
            torch.cuda._sleep(int(0.06 * 2.4e9))
            th0 = time.perf_counter()
            for _ in range(3):
                step()
            host_idle_ms = (time.perf_counter() - th0) / 3 * 1e3
            torch.cuda.synchronize()
        except Exception:  # noqa: BLE001
            host_idle_ms = None
    ddp.agree_on_scan_error()                      # a scan that gave up (on any rank) would make the number meaningless: every rank raises
    allreduce = None
    if world > 1:
        nbytes = ddp._buf.numel() * 4
        ar_ms = algbw = None
        if args.full:
            # the gradient all-reduce alone (same buffer, same communicator), outside the timed region
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(2):
                dist.all_reduce(ddp._buf, op=dist.ReduceOp.SUM)
            fence()
            reps = 10
            ev0.record()
            for _ in range(reps):
                dist.all_reduce(ddp._buf, op=dist.ReduceOp.SUM)
            ev1.record()
            torch.cuda.synchronize()
            ar_ms = ev0.elapsed_time(ev1) / reps
            algbw = nbytes / (ar_ms * 1e-3) / 1e9
        in_step = [a.elapsed_time(b) for a, b in ar_events]
        allreduce = {"bytes": nbytes, "ms": round(ar_ms, 4) if args.full else None,
                     "ms_in_step": round(sum(in_step) / len(in_step), 4) if in_step else None,
                     "ms_in_step_note": "HIP events on the step's stream around poison kernel + collective(s) + dead-rank check, profiled steps only; "
                                        "`ms` (--full) is the same collective back to back after the timed region",
                     "algbw_GBps": round(algbw, 2) if args.full else None,
                     "busbw_GBps": round(algbw * 2 * (world - 1) / world, 2) if args.full else None, "world_size": dist.get_world_size(),
                     "schedule": ("bucket 0 (fusion GRU) early on a communication stream beside backward, the rest + dead slot after backward (M3T_DDP_EARLY_BUCKET=1)"
                                  if getattr(ddp, "_early", False) else
                                  "one all-reduce of the flat buffer after backward" if not ddp.overlap else "3 buckets overlapped with backward"),
                     "xgmi_peak_GBps": 7 * 153.0}
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())

    # ---- roofline of the dominant kernel, from HIP events recorded on the launch stream in the timed region
    kern = {}
    for rec in ops.PROFILE:
        k = kern.setdefault(rec["kernel"], {"ms": 0.0, "launches": 0, "flops": 0.0, "steps": 0, "bytes": 0.0})
        k["ms"] += rec["start"].elapsed_time(rec["end"])
        k["launches"] += rec["launches"]
        k["flops"] += rec["flops"]
        k["bytes"] += rec.get("bytes", 0.0)
        k["steps"] += rec.get("steps", rec["launches"])
    step_ms = dt / args.steps * 1e3
    if os.environ.get("M3T_BENCH_SCAN_TIMELINE") == "1" and ops.PROFILE:
        # debugging: where the scans of the LAST profiled step sit on the device's clock WITHOUT a profiler attached (rocprofv3 slows the
        # host enough to open host-bound holes that the untraced step does not have): offsets from the step's first recorded launch
        recs = [r for r in ops.PROFILE if r["kernel"].startswith("gru_") or r["kernel"] in ("att_fuse_fwd_kernel", "va_loss_kernels")]
        per = len(recs) // max(1, timed_steps)
        last = recs[-per:] if per else []
        if last:
            t0e = last[0]["start"]
            rows = sorted((t0e.elapsed_time(r["start"]), t0e.elapsed_time(r["end"]), r["kernel"]) for r in last)
            prev_end = None
            for a, b, kname in rows:
                print("# tl %8.3f -> %8.3f  %6.3f ms  %s" % (a, b, b - a, kname), file=sys.stderr)
            print("# tl step (first recorded launch to the same launch of the next profiled step is not recorded; ms_per_step %.3f)" % step_ms,
                  file=sys.stderr, flush=True)
    roofline, breakdown = None, {}
    for name, k in kern.items():
        breakdown[name] = {"ms_per_step": round(k["ms"] / timed_steps, 3), "launches_per_step": k["launches"] // timed_steps,
                           "avg_launch_us": round(1e3 * k["ms"] / max(1, k["launches"]), 3),
                           "us_per_time_step": round(1e3 * k["ms"] / max(1, k["steps"]), 3)}
        if k["bytes"] > 0:
            # the small HBM-bound kernels north_star lists (att_fuse: reference models/att_fusion.py:21-25; va_loss: models/utils.py:6-17,
            # models/model.py:132-141): ALGORITHMIC bytes / HIP-event time in the step, against the 8 TB/s HBM peak
            gbps = k["bytes"] / (k["ms"] * 1e-3) / 1e9
            breakdown[name].pop("us_per_time_step")
            breakdown[name].update({"bound": "hbm", "algorithmic_bytes_per_step": int(k["bytes"] / timed_steps), "GBps": round(gbps, 1),
                                    "frac_of_hbm_peak": round(gbps / HBM_PEAK_GBS, 4)})
    name = max((n for n in kern if kern[n]["flops"] > 0), key=lambda n: kern[n]["ms"], default=None)      # (only HBM-bound kernels profiled: no roofline block)
    if name is not None:
        k = kern[name]
        achieved = k["flops"] / (k["ms"] * 1e-3) / 1e12
        traffic, traffic_by_kernel, mfma_util, pmc_source, traffic_ratio = None, None, None, None, None
        # HBM bytes per launch from the committed rocprofv3 PMC passes of this same command (profiles/*pmc_traffic.json: separate
        # FETCH_SIZE / WRITE_SIZE passes, gfx950 correction) and the SQ pass (profiles/*pmc_mfma.json)
        try:
            import glob
            pmc_file = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_traffic.json")))[-1]
            pm = json.load(open(pmc_file))["kernels"]
            stem = name.replace("_kernel", "")               # gru_persist_bwd -> bwd, bwd6, bwd16 variants
            stems = (stem, stem.replace("persist", "solo"))         # the H = 128 levels of the same pass run gru_solo_* launches
            hits = {k: v for k, v in pm.items() if k.startswith(stems) and "hbm_bytes_per_launch" in v}
            if hits:
                traffic = int(sum(h["hbm_bytes_per_launch"] * h["launches"] for h in hits.values()) / sum(h["launches"] for h in hits.values()))
                traffic_by_kernel = {k: v["hbm_bytes_per_launch"] for k, v in hits.items()}
                traffic_ratio = {k: v["traffic_over_algorithmic"] for k, v in hits.items() if "traffic_over_algorithmic" in v} or None
            mfma_file = sorted(glob.glob(os.path.join(ROOT, "profiles", "*pmc_mfma.json")))[-1]
            mm = json.load(open(mfma_file))["kernels"]
            mh = {k: v for k, v in mm.items() if k.startswith(stems) and v.get("mfma_util") is not None}
            if mh:
                mfma_util = {k: v["mfma_util"] for k, v in mh.items()}
            pmc_source = ("profiles/%s and profiles/%s: the builder's committed rocprofv3 --pmc passes of this same command (separate FETCH_SIZE / "
                          "WRITE_SIZE / SQ passes); read from those files, NOT measured in this run"
                          % (os.path.basename(pmc_file), os.path.basename(mfma_file)))
        except Exception:  # noqa: BLE001
            pass
        roofline = {"kernel": name, "bound": "mfma", "achieved": round(achieved, 3), "peak": FP32_MFMA_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                    "avg_launch_us": breakdown[name]["avg_launch_us"],
                    "flops_per_launch": round(k["flops"] / max(1, k["launches"])),
                    "share_of_step": round(k["ms"] / timed_steps / step_ms, 3),
                    "timed_launches": k["launches"], "events_every_n_steps": events_every,
                    "traffic_by_kernel": traffic_by_kernel, "traffic_over_algorithmic_by_kernel": traffic_ratio, "mfma_busy_frac_pmc": mfma_util,
                    "source": {"achieved, avg_launch_us, frac": "HIP events recorded in this run on the launch stream",
                               "traffic, traffic_by_kernel, traffic_over_algorithmic_by_kernel, mfma_busy_frac_pmc": pmc_source},
                    "note": "achieved = algorithmic FLOPs of the recurrent products dh_t = dgh_{t+1} W_hh ((T-1) x sum over scans of 2 B 3H H per launch) / HIP-event "
                            "time of the launches; peak = fp32 MFMA (the arithmetic is fp32-accurate); the H = 512 and H = 256 launches run it as 3 fp16 MFMAs per product "
                            "(two fp16 terms per value, split by the producers; round 4: wide workgroups, 32-deep MFMAs over producer pairs: "
                            "gru_persist_bwd3q_kernel; peak of the 16-bit pipe 2500 TFLOP/s / 3), the H = 128 launches (gru_solo_bwd_kernel) as fp32 FMA chains "
                            "on the vector ALUs; the kernels are bound by the cross-CU exchange latency per time step, not by either pipe (DESIGN.md section 5); "
                            "the audio stack's launches run at the same time as the gru_v | gru_a level's and count with their own event times"}

    if rank == 0:
        clips = B * world * args.steps
        out = {
            "metric": "clips/sec (300-frame A+V, fwd+bwd)", "value": round(clips / dt, 2), "unit": "clips/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(step_ms, 3),
            "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f32 (fp32-accurate products, fp32 accumulate: GEMMs as fp16x3 -- two fp16 terms per scaled operand, three MFMAs, error vs fp64 no larger than an fp32 GEMM's; the forward and backward recurrences at H=512 and H=256 as fp16x3 too (h is bounded; the backward producers split their values under a power-of-two scale per producer workgroup); the H=128 scorer scans as fp32 FMA chains on the vector ALUs)",
            "data": "synthetic",
            "config": {"workload": "C3/C4 feature-level A+V att_fusion graph (SURVEY 8(d)): audio GRU(128,256,2) | "
                                   "gru_v,gru_a GRU(256,512,2) | proj_v | AttFusion([512,512],128) | "
                                   "fusion GRU(512,512,2,9,2); ccc_mtl loss; fwd+bwd+grad-clip"
                                   + ("+RCCL all-reduce" if world > 1 else ""),
                       "clips_per_gpu": B, "global_batch": B * world, "frames": T, "d_audio": d_a, "d_video": d_v,
                       "params": n_params, "parallelism": "dp%d" % world},
            "loss": round(float(loss.detach()), 6),
            "grad_norm": round(float(ddp.last_norm), 6),
            "roofline": roofline,
            "kernels": breakdown,
            "persistent_scan_launches_per_step": persist_per_step,
            "persistent_scan_owner": ops.persist_owner() == 1,
            "host_enqueue_ms_per_step": round(host_ms, 3),
            "host_enqueue_ms_idle": round(host_idle_ms, 3) if host_idle_ms is not None else None,
            "host_enqueue_note": "host_enqueue_ms_per_step = wall time of the timed loop's enqueue calls / steps: it contains the time the host spends "
                                 "blocked behind a full queue (a host that is ahead reads as slow); host_enqueue_ms_idle (--full) = the same step enqueued "
                                 "3 times while the GPU is parked behind a 60 ms spin kernel (no back-pressure): the enqueue path itself",
            "allreduce": allreduce,
            "memory_roofline_frac": round((clips / dt) * 66.15e6 / (HBM_PEAK_GBS * 1e9 * world), 5),
        }
        if dumped is not None:
            out["dump_outputs"] = {"dir": args.dump_outputs, "shapes": dumped}
        if fallback:
            out["fallback"] = ("launch-per-step scans + gradient buckets overlapped with backward, in fresh worker processes, after: %s"
                               % fallback)
        out["cpu_baseline"] = None
        if args.full and world == 1 and not args.no_cpu_baseline:
            print("# gpu leg done: %.2f clips/s, %.3f ms/step; timing the CPU baseline ..." % (out["value"], step_ms),
                  file=sys.stderr, flush=True)
            try:
                out["cpu_baseline"] = cpu_baseline(args.cpu_clips, T, d_a, d_v)
                out["speedup_vs_cpu"] = round(out["value"] / out["cpu_baseline"]["value"], 1)
            except Exception as e:  # noqa: BLE001
                out["cpu_baseline_error"] = repr(e)
        if args.full and world == 1 and args.aux:
            print("# timing the secondary configs (%s) ..." % args.aux, file=sys.stderr, flush=True)
            try:
                out["aux"] = run_aux(args.aux, args.aux_budget)
            except Exception as e:  # noqa: BLE001
                out["aux"] = {"note": repr(e)}
        # the secondary configs' step times once more, compact: right behind ms_per_step AND as the last key of the line (whichever end of
        # a long line a log keeps -- VERDICT r4 weak-9: the driver's tail is 2000 characters)
        if isinstance(out.get("aux"), dict):
            brief = {k: v.get("ms_per_step") for k, v in out["aux"].items() if isinstance(v, dict) and v.get("ms_per_step") is not None}
            if brief:
                out = {k2: v2 for k, v in out.items() for k2, v2 in (((k, v), ("aux_ms", brief)) if k == "ms_per_step" else ((k, v),))}
                out["aux_ms_per_step"] = brief
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
