#!/usr/bin/env python3
"""Time the batched JPEG decode (m3t.jpeg, csrc/jpeg.hip) on one MI355X.  The batch is the 256 x 256 quality-95 4:2:0 fixture of
tests/golden/jpeg_cases.npz replicated; for each frame count (default 512 = one C5 step, 3072 = the reference's default batch):

  pack           host: jpeg.pack of the files' bytes (header walk, restart scan, tables) into the pinned stream buffer
  copy           the stream buffer, pinned host -> device
  device_decode  m3t_jpeg_decode_walk on device-resident inputs: all launches (entropy + IDCT, then upsampling + colour), once with the
                 sequential walk (the yardstick: m3t_jpeg_decode's kernel) and once with the parallel walk (--sub-bytes, --lanes)
  decode         jpeg.decode as a caller sees it: table copy + stream copy + the launches, for both walks
  pillow_16      where Pillow imports: the same frames decoded on the host by 16 threads (Image.open(...).convert("RGB"))

With --sweep, in front of that: at the first frame count, the sequential walk and the parallel walk at every sub-sequence size of
--sweep-sub and every workgroup size of --sweep-lanes, all alternately in one process, with the median exchange passes from the walk
stats -- the table jpeg.AUTO_SUB_BYTES and jpeg.AUTO_MIN_BYTES are picked from.

Then the C5 training step of tools/ingest_bench.py --input-size 256 fed three ways, alternately in one process: from a ready pinned
uint8 batch (that tool's c5_step_u8), and from JPEG bytes by either walk -- the next step's decode issued on a side stream before the
step, then video.ingest.  Each sample is a host clock around `--inner` repetitions that end in a device synchronise; medians and the
spread are printed as one JSON line.

With --crossover, in front of everything: 512 copies of each small fixture (0.5 to 4 KB a segment) by the sequential walk and by the
parallel walk at sub-sequences of 64 and 256 bytes -- where the workgroup's fixed costs (tables into LDS, the barriers of eight phases)
stop paying, which is what jpeg.AUTO_MIN_BYTES is picked from.

    python tools/jpeg_bench.py [--frames 512 3072] [--samples 11] [--inner 3] [--step-samples 9] [--no-step]
                               [--sub-bytes 256] [--lanes 256] [--sweep] [--sweep-sub 64 128 256 512] [--sweep-lanes 64 128 256] [--crossover]
"""
import argparse
import io
import json
import os
import random
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "m3f.pytorch_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from ingest_bench import alternate, summary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, nargs="+", default=[512, 3072])
    ap.add_argument("--samples", type=int, default=11)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--step-samples", type=int, default=9)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--sub-bytes", type=int, default=None, help="the parallel walk's sub-sequence (default: jpeg.AUTO_SUB_BYTES)")
    ap.add_argument("--lanes", type=int, default=None, help="the parallel walk's workgroup size (default: the library's)")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-sub", type=int, nargs="+", default=[64, 128, 256, 512])
    ap.add_argument("--sweep-lanes", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--crossover", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_bench needs the GPU: a timing taken anywhere else says nothing")
    from m3t import _lib, jpeg, video
    dev = torch.device("cuda", 0)
    lib = _lib.load()
    data = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"))["full_256_q95.jpg"].tobytes()
    sub_bytes = a.sub_bytes or jpeg.AUTO_SUB_BYTES
    if a.lanes:
        jpeg.par_lanes(a.lanes)
    lanes = jpeg.par_lanes()
    out = {"tool": "jpeg_bench", "fixture_bytes": len(data), "sub_bytes": sub_bytes, "lanes": lanes, "sizes": {}}
    try:
        from PIL import Image
    except ImportError:
        Image = None

    if a.crossover:
        small = dict(np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz")))
        small.update(np.load(os.path.join(ROOT, "tests", "golden", "jpeg_par_cases.npz")))
        rows = []
        if Image is not None:                               # the sizes between the fixtures and the dataset's frame: its centre, cropped
            full = Image.open(io.BytesIO(data)).convert("RGB")
            for side in (64, 96, 128, 192):
                buf = io.BytesIO()
                full.crop((128 - side // 2, 128 - side // 2, 128 + side // 2, 128 + side // 2)).save(buf, "JPEG", quality=95, subsampling=2)
                small["crop_%d_q95.jpg" % side] = np.frombuffer(buf.getvalue(), np.uint8)
        for name in ["f_gray_q80", "f_444_q60", "f_422_q85", "f_420_q95", "p_422_opt_q97", "p_noise_444_q100"] + \
                    sorted((k[:-4] for k in small if k.startswith("crop_")), key=lambda k: int(k.split("_")[1])):
            b = jpeg.pack([small[name + ".jpg"].tobytes()] * 512, pin=True)
            fns = [lambda w=w, sb=sb: jpeg.decode(b, walk=w, sub_bytes=sb) for w, sb in (("sequential", 64), ("parallel", 64), ("parallel", 256))]
            t = alternate(fns, a.samples, a.inner)
            rows.append({"case": name, "segment_bytes": int(b.segments[0, 2]), "size": [b.height, b.width], "sequential": summary(t[0]),
                         "parallel_64": summary(t[1]), "parallel_256": summary(t[2])})
        out["crossover"] = {"frames": 512, "what": "jpeg.decode (copies included)", "rows": rows}

    for n in a.frames:
        items = [data] * n
        packs = []
        for _ in range(3):
            t0 = time.perf_counter()
            b = jpeg.pack(items, pin=True)
            packs.append((time.perf_counter() - t0) * 1e3)
        H, W = b.height, b.width
        tables = np.ascontiguousarray(b.tables, np.int32)
        t_d = torch.from_numpy(tables).to(dev)
        s_d = b.stream.to(dev)
        frames = torch.empty(n, H, W, 3, dtype=torch.uint8, device=dev)
        ws = torch.empty(int(lib.m3t_jpeg_workspace_bytes(n, H, W)), dtype=torch.uint8, device=dev)
        status = torch.empty(n, dtype=torch.int32, device=dev)

        stats = torch.zeros(b.n_segs, 2, dtype=torch.int32, device=dev)

        def device_decode(walk, sub=sub_bytes, wg=lanes):
            def run():
                lib.m3t_jpeg_par_lanes(wg)
                _lib.check(lib.m3t_jpeg_decode_walk(s_d.data_ptr(), s_d.numel(), tables.ctypes.data, t_d.data_ptr(), n, b.n_segs, b.n_quant,
                                                    b.n_huff, H, W, frames.data_ptr(), n, 0, ws.data_ptr(), ws.numel(), status.data_ptr(),
                                                    walk, sub, 0, 1 << 30, stats.data_ptr(), torch.cuda.current_stream().cuda_stream),
                           "m3t_jpeg_decode_walk")
            return run

        def copy():
            return b.stream.to(dev, non_blocking=True)

        def decode(walk):
            return lambda: jpeg.decode(b, walk=walk, sub_bytes=sub_bytes)

        if a.sweep and n == a.frames[0]:
            # every configuration alternately in one process; the reference frames come from the sequential walk
            device_decode(0)()
            want = frames.clone()
            grid = [(sub, wg) for wg in a.sweep_lanes for sub in a.sweep_sub]
            t = alternate([device_decode(0)] + [device_decode(1, sub, wg) for sub, wg in grid], a.samples, a.inner)
            sweep = {"frames": n, "sequential": summary(t[0]), "parallel": []}
            for (sub, wg), ts in zip(grid, t[1:]):
                device_decode(1, sub, wg)()
                torch.cuda.synchronize()
                assert torch.equal(frames, want) and not status.any().item()
                st = stats.cpu().numpy()
                sweep["parallel"].append(dict(summary(ts), sub_bytes=sub, lanes=wg, sub_sequences=int(st[0, 0]), passes_median=float(np.median(st[:, 1])),
                                              passes_max=int(st[:, 1].max())))
            lib.m3t_jpeg_par_lanes(lanes)
            out["sweep"] = sweep

        t = alternate([device_decode(0), device_decode(1), copy, decode("sequential"), decode("parallel")], a.samples, a.inner)
        assert not status.any().item()
        row = {"pack_host": summary(packs), "copy": summary(t[2]), "device_decode": summary(t[0]), "device_decode_parallel": summary(t[1]),
               "decode": summary(t[3]), "decode_parallel": summary(t[4]), "stream_bytes": int(b.stream.numel()), "segments": b.n_segs}
        if Image is not None:
            def one(_):
                return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
            with ThreadPoolExecutor(16) as pool:
                ts = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    list(pool.map(one, range(n), chunksize=16))
                    ts.append((time.perf_counter() - t0) * 1e3)
            row["pillow_16"] = summary(ts)
        out["sizes"][str(n)] = row
        del frames, ws, s_d

    if not a.no_step:
        from m3t.ddp import FlatGradDDP
        from models.model import AffWild2VA
        N, T = 8, 64
        rs = np.random.RandomState(0)
        random.seed(0)
        np.random.seed(0)
        aug = [video.draw_affwild(256, True, True, True, random.random() > 0.5, resize=True) for _ in range(N)]
        ready = torch.from_numpy(rs.randint(0, 256, (N, T, 256, 256, 3)).astype(np.uint8)).pin_memory()
        b = jpeg.pack([data] * (N * T), pin=True)
        hp = AffWild2VA.add_model_specific_args(argparse.ArgumentParser(add_help=False)).parse_args([])
        hp.modality, hp.fusion_type, hp.loss, hp.window = "audiovisual", "attention", "ccc_mtl", T
        torch.manual_seed(12345)
        m = AffWild2VA(hp).to(dev).train()
        f = lambda arr: torch.from_numpy(arr).to(dev)
        rest = {"se_features": f(rs.standard_normal((N, 512, T)).astype(np.float32)), "audio": f(rs.standard_normal((N, T, 200)).astype(np.float32)),
                "label_valence": f(rs.uniform(-1, 1, (N, T)).astype(np.float32)), "label_arousal": f(rs.uniform(-1, 1, (N, T)).astype(np.float32)),
                "class_expr": f(rs.randint(0, 7, (N, T)).astype(np.int64)), "expr_valid": f(rs.uniform(size=(N, T)) < 0.7)}
        ddp = FlatGradDDP(m, max_norm=1.0)
        side = torch.cuda.Stream(dev)

        def step(batch):
            ddp.zero_grad()
            m.training_step(batch, 0)["loss"].backward()
            ddp.finish()

        def issue_decode(walk):
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fr, st = jpeg.decode(b, walk=walk, sub_bytes=sub_bytes)
                ev = torch.cuda.Event()
                ev.record(side)
            return fr, st, ev

        def jpeg_step(walk):
            state = [issue_decode(walk)]

            def run():
                fr, st, ev = state[0]
                torch.cuda.current_stream().wait_event(ev)
                fr.record_stream(torch.cuda.current_stream())
                state[0] = issue_decode(walk)                # the next step's frames decode beside this step
                step(dict(rest, video=fr.view(N, T, 256, 256, 3), video_aug=aug))
            return run

        def u8_step():
            step(dict(rest, video=ready, video_aug=aug))

        steps = alternate([u8_step, jpeg_step("sequential"), jpeg_step("parallel")], a.step_samples, 3)
        out["c5_step_u8_ready"] = summary(steps[0])
        out["c5_step_from_jpeg"] = summary(steps[1])
        out["c5_step_from_jpeg_parallel"] = summary(steps[2])
    out["note"] = ("pinned host buffers -> device; device_decode = both launches on resident inputs; decode = jpeg.decode (copies included); "
                   "*_parallel = the same with the parallel walk; c5_step_from_jpeg = AffWild2VA training step (training_step + backward + clip) whose frames were decoded on a side stream "
                   "while the previous step ran, against the same step fed a ready pinned uint8 batch; alternately in one process, "
                   "%d samples x %d calls (steps: %d x 3)" % (a.samples, a.inner, a.step_samples))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
