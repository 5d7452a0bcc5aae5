"""numpy restatement of the baseline-JPEG decoding rules (include/m3t_hip.h, m3t_jpeg_decode; libjpeg's jdhuff.c, jidctint.c, jdsample.c,
jdcolor.c), shared by tests/test_jpeg_host.py, tests/test_gpu_jpeg.py and tests/golden/gen_golden_jpeg.py.  It has its own header walk and
shares no code with m3t/jpeg.py.  decode(data) -> (rgb uint8 [H, W, 3], stats); it raises DecodeError wherever a stream is not a
complete, valid one (truncated, no such code, a coefficient past 63, a wrong or missing restart marker, bytes left over)."""
import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]


class DecodeError(ValueError):
    pass


def read_header(data):
    """-> dict: H, W, comps [(id, h, v, tq)], quant {id: [64] zig-zag}, huff {(class, id): {(length, code): symbol}}, ri, scan (bytes up to EOI)"""
    assert data[:2] == b"\xff\xd8"
    p, quant, huff, ri, frame = 2, {}, {}, 0, None
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        n = (data[p + 2] << 8) | data[p + 3]
        body = data[p + 4:p + 2 + n]
        if m == 0xDB:
            q = 0
            while q < len(body):
                assert body[q] >> 4 == 0
                quant[body[q] & 15] = list(body[q + 1:q + 65])
                q += 65
        elif m == 0xC4:
            q = 0
            while q < len(body):
                counts = list(body[q + 1:q + 17])
                syms = body[q + 17:q + 17 + sum(counts)]
                table, code, k = {}, 0, 0
                for length in range(1, 17):
                    for _ in range(counts[length - 1]):
                        table[(length, code)] = syms[k]
                        code += 1
                        k += 1
                    code <<= 1
                huff[(body[q] >> 4, body[q] & 15)] = table
                q += 17 + sum(counts)
        elif m == 0xC0:
            frame = body
        elif m == 0xDD:
            ri = (body[0] << 8) | body[1]
        elif m == 0xDA:
            break
        else:
            assert 0xE0 <= m <= 0xEF or m == 0xFE, hex(m)
        p += 2 + n
    assert frame[0] == 8
    H, W, nc = (frame[1] << 8) | frame[2], (frame[3] << 8) | frame[4], frame[5]
    comps = [(frame[6 + 3 * c], frame[7 + 3 * c] >> 4, frame[7 + 3 * c] & 15, frame[8 + 3 * c]) for c in range(nc)]
    assert body[0] == nc
    tabs = [(body[2 + 2 * c] >> 4, body[2 + 2 * c] & 15) for c in range(nc)]
    return {"H": H, "W": W, "comps": comps, "quant": quant, "huff": huff, "tabs": tabs, "ri": ri, "scan": data[p + 2 + n:]}


class _Bits:
    def __init__(self, data):
        self.d, self.p, self.buf, self.cnt = data, 0, 0, 0

    def bit(self):
        if self.cnt == 0:
            if self.p >= len(self.d):
                raise DecodeError("truncated")
            b = self.d[self.p]
            self.p += 1
            if b == 0xFF:
                if self.p >= len(self.d) or self.d[self.p] != 0:
                    raise DecodeError("a marker inside the entropy-coded data")
                self.p += 1
            self.buf, self.cnt = b, 8
        self.cnt -= 1
        return (self.buf >> self.cnt) & 1

    def bits(self, n):
        v = 0
        for _ in range(n):
            v = (v << 1) | self.bit()
        return v

    def symbol(self, table, stats):
        code = 0
        for length in range(1, 17):
            code = (code << 1) | self.bit()
            s = table.get((length, code))
            if s is not None:
                stats["max_code_length"] = max(stats["max_code_length"], length)
                return s
        raise DecodeError("no such Huffman code")


def _extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def _idct_1d(c, shift):
    """c: int64 [..., 8] -> [..., 8]; the values stay inside 32 bits for every valid stream"""
    c0, c1, c2, c3, c4, c5, c6, c7 = (c[..., i] for i in range(8))
    z1 = (c2 + c6) * 4433
    t2 = z1 - c6 * 15137
    t3 = z1 + c2 * 6270
    t0 = (c0 + c4) << 13
    t1 = (c0 - c4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = c7, c5, c3, c1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * 9633
    t0, t1, t2, t3 = t0 * 2446, t1 * 16819, t2 * 25172, t3 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3], axis=-1)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return (out + (1 << (shift - 1))) >> shift


def idct_blocks(coef, q):
    """coef int [n, 8, 8] (natural order), q [8, 8] -> samples before the clamp, int64 [n, 8, 8] (+128 added)"""
    x = coef.astype(np.int64) * np.asarray(q, np.int64)
    ws = _idct_1d(x.transpose(0, 2, 1), 11).transpose(0, 2, 1)        # columns
    return _idct_1d(ws, 18) + 128                                      # rows


def upsample(p, hs, vs, H, W):
    """p: the component's real-size plane [ch, cw] -> [H, W] by libjpeg's fancy upsampling"""
    ch, cw = p.shape
    p = p.astype(np.int64)
    if hs == 1 and vs == 1:
        return p[:H, :W]
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)[:H, :W]
    if vs == 1:
        out = np.empty((ch, 2 * cw), np.int64)
        left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
        right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
        out[:, 0::2] = (3 * p + left + 1) >> 2
        out[:, 1::2] = (3 * p + right + 2) >> 2
        out[:, 0] = p[:, 0]
        out[:, -1] = p[:, -1]
        return out[:H, :W]
    out = np.empty((2 * ch, 2 * cw), np.int64)
    for v in (0, 1):
        nb = np.clip(np.arange(ch) + (1 if v else -1), 0, ch - 1)
        s = 3 * p + p[nb]
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        o = np.empty((ch, 2 * cw), np.int64)
        o[:, 0::2] = (3 * s + left + 8) >> 4
        o[:, 1::2] = (3 * s + right + 7) >> 4
        out[v::2] = o
    return out[:H, :W]


def decode(data):
    """bytes -> (rgb uint8 [H, W, 3], stats {zrl, max_code_length, restarts, clamp_low, clamp_high})"""
    h = read_header(bytes(data))
    H, W, comps = h["H"], h["W"], h["comps"]
    nc = len(comps)
    assert nc in (1, 3)
    hs, vs = (1, 1) if nc == 1 else (comps[0][1], comps[0][2])
    assert (hs, vs) in ((1, 1), (2, 1), (2, 2)) and all(c[1] == 1 and c[2] == 1 for c in comps[1:])
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    fac = [(hs, vs)] + [(1, 1)] * (nc - 1)
    coefs = [np.zeros((my * v, mx * f, 64), np.int64) for f, v in fac]
    stats = {"zrl": 0, "max_code_length": 0, "restarts": 0, "clamp_low": 0, "clamp_high": 0}
    scan = h["scan"]
    # cut the scan at its markers: RSTn between intervals, EOI at the end
    pieces, marks, start, i = [], [], 0, 0
    while True:
        i = scan.find(b"\xff", i)
        if i < 0 or i + 1 >= len(scan):
            raise DecodeError("no EOI marker")
        m = scan[i + 1]
        if m == 0:
            i += 2
            continue
        pieces.append(scan[start:i])
        marks.append(m)
        if not 0xD0 <= m <= 0xD7:
            break
        start = i = i + 2
    if marks[-1] != 0xD9:
        raise DecodeError("marker 0x%02X inside the scan" % marks[-1])
    ri = h["ri"] if h["ri"] else mx * my
    want = -(-(mx * my) // ri)
    if len(pieces) != want or any(marks[k] != 0xD0 + (k & 7) for k in range(want - 1)):
        raise DecodeError("restart markers: %d intervals, markers %s" % (len(pieces), [hex(m) for m in marks]))
    stats["restarts"] = want - 1
    for k, piece in enumerate(pieces):
        rd = _Bits(piece)
        pred = [0] * nc
        for m in range(k * ri, min((k + 1) * ri, mx * my)):
            r0, c0 = divmod(m, mx)
            for c in range(nc):
                dc_t, ac_t = h["huff"][(0, h["tabs"][c][0])], h["huff"][(1, h["tabs"][c][1])]
                f, v = fac[c]
                for bv in range(v):
                    for bh in range(f):
                        blk = coefs[c][r0 * v + bv, c0 * f + bh]
                        s = rd.symbol(dc_t, stats)
                        if s > 15:
                            raise DecodeError("DC size")
                        pred[c] += _extend(rd.bits(s), s)
                        blk[0] = pred[c]
                        kk = 1
                        while kk < 64:
                            rs = rd.symbol(ac_t, stats)
                            run, s = rs >> 4, rs & 15
                            if s == 0:
                                if run != 15:
                                    break
                                stats["zrl"] += 1
                                kk += 16
                                continue
                            kk += run
                            if kk >= 64:
                                raise DecodeError("a coefficient past the block")
                            blk[ZIGZAG[kk]] = _extend(rd.bits(s), s)
                            kk += 1
        if rd.p < len(piece):
            raise DecodeError("bytes left in a segment")
    planes = []
    for c in range(nc):
        q = np.zeros(64, np.int64)
        q[ZIGZAG] = h["quant"][comps[c][3]]
        rows, cols = coefs[c].shape[:2]
        s = idct_blocks(coefs[c].reshape(-1, 8, 8), q.reshape(8, 8)).reshape(rows, cols, 8, 8)
        stats["clamp_low"] += int((s < 0).sum())
        stats["clamp_high"] += int((s > 255).sum())
        planes.append(np.clip(s, 0, 255).transpose(0, 2, 1, 3).reshape(rows * 8, cols * 8))
    Y = planes[0][:H, :W]
    if nc == 1:
        return np.repeat(Y[:, :, None], 3, axis=2).astype(np.uint8), stats
    cw, ch = -(-W // hs), -(-H // vs)
    cb = upsample(planes[1][:ch, :cw], hs, vs, H, W) - 128
    cr = upsample(planes[2][:ch, :cw], hs, vs, H, W) - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=2), 0, 255).astype(np.uint8), stats
