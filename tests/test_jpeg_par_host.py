"""The parallel walk of the JPEG decode without a GPU: csrc/jpeg_par.h compiled for the host by csrc/jpeg_host_check.cpp (its seven-argument
form), which calls the phases of jpeg_par_kernel -- the same functions, on the kernel's own data layout -- for one lane after the other.
Every golden of both fixture files bit for bit at three sub-sequence sizes and two lane
counts, the fixed-seed damaged streams against the sequential walk of the same program (frames AND status words equal: a segment with a
marker inside takes its status from the sequential reader, so the walks never differ, not even in the RST bit), guard bytes around
everything the emulated workgroup writes, the refusals, and the same program under the address and undefined-behaviour sanitizers."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import load_golden
import jpeg_cases
import jpeg_ref
from m3t import jpeg, _lib

CASES, _ = jpeg_cases.load()
EINVAL_EXIT = 2                                    # the program's exit code for what m3t_jpeg_decode_walk answers with M3T_EINVAL


@functools.lru_cache(None)
def par_cases():
    d = load_golden("jpeg_par_cases")
    return {k[:-4]: (d[k].tobytes(), d[k[:-4] + ".rgb"]) for k in d if k.endswith(".jpg")}


def all_cases():
    out = dict(CASES)
    out.update(par_cases())
    return out


def by_size():
    groups = {}
    cases = all_cases()
    for name in sorted(cases):
        groups.setdefault(cases[name][1].shape[:2], []).append(name)
    return groups


def _build(tmp_path_factory, flags):
    exe = str(tmp_path_factory.mktemp("jpeg_par") / "jpeg_host_check")
    subprocess.check_call(["g++"] + flags + [os.path.join(_lib.CSRC_DIR, "jpeg_host_check.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def par_check(tmp_path_factory):
    return _build(tmp_path_factory, ["-O2", "-Wall", "-Werror"])


def run(exe, tmp_path, items, walk=1, sub_bytes=32, par_min=0, par_max=1 << 30, lanes=64, order="bgr", env=None):
    """decode `items` into every second frame of a canary-filled destination -> (status [n], frames [n, H, W, 3] rgb, stats [n_segs, 2],
    the raw bytes of the result file, stderr)"""
    b = jpeg.pack(items)
    n = b.n
    slots = 2 * np.arange(n) + 1
    src, dst = str(tmp_path / "packed.bin"), str(tmp_path / "out.bin")
    jpeg_cases.write_packed(src, b, slots, 2 * n + 1, order)
    r = subprocess.run([exe, src, dst, str(walk), str(sub_bytes), str(par_min), str(par_max), str(lanes)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr)
    status, frames = jpeg_cases.read_result(dst, n, 2 * n + 1, b.height, b.width)
    assert (frames[0::2] == jpeg_cases.CANARY).all(), "a frame nobody named was written"
    stats = np.fromfile(dst + ".stats", "<i4").reshape(b.n_segs, 2)
    out = frames[1::2]
    with open(dst, "rb") as f:
        raw = f.read()
    return status, (out[..., ::-1] if order == "bgr" else out), stats, raw, r.stderr, b


def check_stats(stats, taken):
    """(sub-sequences, passes): 1 <= passes <= sub-sequences where the parallel walk took the segment, (0, 0) elsewhere"""
    taken = np.asarray(taken, bool)
    assert (stats[~taken] == 0).all()
    assert (stats[taken, 1] >= 1).all() and (stats[taken, 1] <= stats[taken, 0]).all(), stats[taken]


def test_the_new_fixtures_equal_the_restatement():
    for name, (data, rgb) in sorted(par_cases().items()):
        assert np.array_equal(jpeg_ref.decode(data)[0], rgb), name
    assert sorted(par_cases()) == ["p_422_opt_q97", "p_flat_420_q30", "p_gray_odd_q92", "p_noise_444_q100", "p_ramp_420_q75", "p_rows_420_rst"]
    assert jpeg.pack([par_cases()["p_rows_420_rst"][0]]).n_segs == 4


@pytest.mark.parametrize("lanes", [64, 256])
@pytest.mark.parametrize("sub_bytes", [16, 32, 256])
def test_parallel_walk_reproduces_every_golden(par_check, tmp_path, sub_bytes, lanes):
    cases = all_cases()
    groups = by_size()
    assert len(groups[(40, 56)]) == 8 and len(cases) == len(CASES) + 6
    for k, (size, names) in enumerate(sorted(groups.items())):
        status, rgb, stats, _, _, b = run(par_check, tmp_path, [cases[n][0] for n in names], sub_bytes=sub_bytes, lanes=lanes,
                                          order="rgb" if k % 2 else "bgr")
        assert not status.any(), (names, status)
        for i, n in enumerate(names):
            assert np.array_equal(rgb[i], cases[n][1]), n
        check_stats(stats, np.ones(b.n_segs, bool))
        if names == ["full_256_q95"] and sub_bytes == 16:
            assert stats[0, 0] > 2048                                     # more sub-sequences than any lane count: a lane takes several


def test_results_do_not_depend_on_the_split(par_check, tmp_path):
    """stats differ with sub_bytes, frames and status may not; the sub-sequence count does not depend on the lane count at all"""
    items = [all_cases()[n][0] for n in jpeg_cases.FAMILY]
    ref = run(par_check, tmp_path, items, walk=0)
    assert (ref[2] == 0).all()
    for sub_bytes, lanes in ((16, 1), (48, 7), (64, 64), (4096, 1024)):
        got = run(par_check, tmp_path, items, sub_bytes=sub_bytes, lanes=lanes)
        assert got[3] == ref[3], (sub_bytes, lanes)
        again = run(par_check, tmp_path, items, sub_bytes=sub_bytes, lanes=64)
        assert np.array_equal(got[2], again[2])


def test_routing_by_segment_bytes(par_check, tmp_path):
    names = jpeg_cases.FAMILY
    items = [CASES[n][0] for n in names]
    status, rgb, stats, _, _, b = run(par_check, tmp_path, items, par_min=1000, par_max=1500)
    assert not status.any()
    for i, n in enumerate(names):
        assert np.array_equal(rgb[i], CASES[n][1]), n
    taken = (b.segments[:, 2] >= 1000) & (b.segments[:, 2] <= 1500)
    assert taken.any() and not taken.all()
    check_stats(stats, taken)
    assert (stats[taken, 0] >= 1).all()


def test_damaged_streams_equal_the_sequential_walk(par_check, tmp_path):
    items, names = jpeg_cases.damaged_batch()
    seq = run(par_check, tmp_path, items, walk=0)
    par = run(par_check, tmp_path, items, walk=1, sub_bytes=32)
    # the contract allows the RST bit to differ where a marker lies past the last consumed bit; this walk takes the status of such a
    # segment from the sequential reader, so the list of permitted exceptions is empty and the result files are equal byte for byte
    assert par[3] == seq[3]
    count = jpeg_cases.check_damaged_result(names, par[1], par[0])
    print(count)
    assert count["flagged"] >= 22 and count["neighbour"] >= 28
    check_stats(par[2], np.ones(par[5].n_segs, bool))
    for sub_bytes, lanes in ((16, 256), (256, 64)):
        assert run(par_check, tmp_path, items, sub_bytes=sub_bytes, lanes=lanes)[3] == seq[3]


def test_markers_inside_a_segment(par_check, tmp_path):
    """FF followed by a non-zero byte, and FF as a segment's last byte, at the front, the middle and the end of a scan: pack passes such
    bytes on (FF FF is no marker to the header walk), the walks must agree on frames and on every status bit"""
    head, scan, tail = jpeg_cases.split(CASES["f_420_q95"][0])
    items = [CASES["f_420_q95"][0]]
    for at in (0, 1, 17, len(scan) // 2, len(scan) - 40, len(scan) - 6, len(scan) - 3, len(scan) - 2):
        b = bytearray(scan)
        b[at:at + 3] = b"\xff\xff\x00"                                   # (FF FF 00: the header walk reads a fill byte and a stuffed FF)
        items.append(head + bytes(b) + tail)
    for cut in (1, 300, len(scan) - 1):
        items.append(head + scan[:cut] + b"\xff" + tail)                  # a lone FF closes the segment
    for it in items:
        jpeg.parse(it)
    seq = run(par_check, tmp_path, items, walk=0)
    assert seq[0][0] == 0 and (seq[0][1:] != 0).all()
    for sub_bytes in (16, 64):
        assert run(par_check, tmp_path, items, sub_bytes=sub_bytes)[3] == seq[3]


def test_bad_walk_arguments_exit_with_einval(par_check, tmp_path):
    b = jpeg.pack([CASES["f_420_q95"][0]])
    src = str(tmp_path / "packed.bin")
    jpeg_cases.write_packed(src, b, np.arange(1), 1, "bgr")

    def rc(walk, sub_bytes):
        return subprocess.run([par_check, src, str(tmp_path / "o.bin"), str(walk), str(sub_bytes), "0", "65536", "64"], capture_output=True).returncode

    assert rc(1, 32) == 0 and rc(0, 4096) == 0
    for walk, sub_bytes in ((1, 0), (1, 24), (1, 8192), (1, 8), (1, -16), (2, 32), (-1, 32)):
        assert rc(walk, sub_bytes) == EINVAL_EXIT, (walk, sub_bytes)


def test_under_the_sanitizers(tmp_path_factory, tmp_path):
    """the same text with -fsanitize=address,undefined, run as a plain executable: the goldens and the damaged batch, a clean exit and
    nothing on stderr"""
    probe = str(tmp_path / "probe.cpp")
    with open(probe, "w") as f:
        f.write("int main() { return 0; }\n")
    # the runtimes are linked statically, so the executable does not care what else the process loads
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-Wall", "-Werror"]
    if subprocess.run(["g++"] + flags + [probe, "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the compiler has no sanitizer runtime")
    exe = _build(tmp_path_factory, flags)
    env = None
    cases = all_cases()
    for size, names in sorted(by_size().items()):
        sub_bytes = 256 if names == ["full_256_q95"] else 16
        status, rgb, _, _, err, _ = run(exe, tmp_path, [cases[n][0] for n in names], sub_bytes=sub_bytes, lanes=64, env=env)
        assert err == "" and not status.any()
        for i, n in enumerate(names):
            assert np.array_equal(rgb[i], cases[n][1]), n
    items, names = jpeg_cases.damaged_batch()
    seq = run(exe, tmp_path, items, walk=0, env=env)
    par = run(exe, tmp_path, items, walk=1, sub_bytes=32, env=env)
    assert seq[4] == "" and par[4] == "" and par[3] == seq[3]
