// Video ingest on the GPU: everything the reference's two loaders do to pixels between the decoder and the first convolution
// (models/dataset.py:16-31,46-80 and :312, models/vox2_dataset.py:14-50, models/cv_augment.py:6-37, models/model.py:106) in one pass
// over the uint8 frames as decoded, [N][Ts][Hs][Ws][3] channels-last:
//     f = frame_idx[n][t]                                   (-1: no frame yet -> zeros; repeats and edge padding are index repeats)
//     v = f < 0 ? 0 : frames[n][f][cy + y][cx + (mirror ? W-1-x : x)][c]
//     o = (y, x) inside the clip's cutout ? 0.0f : lut[n][v]
// The 256-entry table carries normalisation and the VoxCeleb2 colour jitter (two uint8 tables composed in front of it), so the kernel
// only gathers: its values are the table's bits.  One workgroup takes R output rows of one frame: the source bytes of the cropped
// row segments come in as 16-byte granules (3 cx is not 4-aligned in general: each row is fetched from its 16-byte floor and picked
// apart from LDS), the table sits in LDS beside them.  Layout 0 writes the four-channel rows the first layers' tap walk reads
// (conv3d.hip, m3t_planes_to_cl4's image) and raises the pending magnitude slot; layout 1 writes channel planes.
#include "common.h"

namespace {

struct IngestArgs {
    const uint8_t* frames; const int* frame_idx; const int* geom; const float* lut; float* out; unsigned long long* slot;
    long long bytes, units;          // bytes of `frames`; units = N T tiles
    int Ts, Hs, Ws, T, H, W, lut_stride, layout, R, G, tiles;
};

// LDS: 256 floats of table | R rows of (G + 1) granules (the extra one: the two-dword pick of a row's last pixel may touch it)
__global__ __launch_bounds__(256) void video_ingest_kernel(IngestArgs a) {
    extern __shared__ uint4 smem[];
    float* lut = reinterpret_cast<float*>(smem);
    uint4* raw = smem + 64;
    const unsigned* raw32 = reinterpret_cast<const unsigned*>(raw);
    const int tid = threadIdx.x, H = a.H, W = a.W, G = a.G, GS = a.G + 1;
    const long long HW = (long long)H * W;
    float mx = 0.f;
    for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const long long nt = unit / a.tiles;
        const int tile = (int)(unit - nt * a.tiles);
        const int n = (int)(nt / a.T), t = (int)(nt - (long long)n * a.T);
        const int y0 = tile * a.R, rows = min(a.R, H - y0);
        const int* g = a.geom + 8 * (long long)n;
        // a bad device-side table cannot leave the allocation: window and frame index are clamped into range
        const int cy = min(max(g[0], 0), a.Hs - H), cx = min(max(g[1], 0), a.Ws - W), mirror = g[2];
        const int ky1 = g[3], ky2 = g[4], kx1 = g[5], kx2 = g[6];
        int f = a.frame_idx ? a.frame_idx[(long long)n * a.T + t] : t;
        const bool blank = f < 0;
        f = min(max(f, 0), a.Ts - 1);
        const long long row_bytes = 3ll * a.Ws;
        const long long base0 = ((((long long)n * a.Ts + f) * a.Hs + cy + y0) * a.Ws + cx) * 3;      // first byte of the tile's first row segment
        __syncthreads();                                     // (the previous unit's picks are done)
        lut[tid] = a.lut[(long long)n * a.lut_stride + tid];
        if (!blank) {
            for (int i = tid; i < rows * G; i += 256) {
                const int r = i / G, q = i - r * G;
                const long long b = base0 + r * row_bytes, o = (b & ~15ll) + 16ll * q;
                if (o >= b + 3ll * W) continue;              // (a granule past the segment: never picked from)
                uint4 v;
                if (o + 16 <= a.bytes) {
                    v = *reinterpret_cast<const uint4*>(a.frames + o);
                } else {                                     // the allocation's last, partial granule: byte by byte
                    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        if (o + k < a.bytes) w[k >> 2] |= (unsigned)a.frames[o + k] << (8 * (k & 3));
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                raw[r * GS + q] = v;
            }
        }
        __syncthreads();
        for (int p = tid; p < rows * W; p += 256) {
            const int r = p / W, x = p - r * W, y = y0 + r;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!(y >= ky1 && y < ky2 && x >= kx1 && x < kx2)) {
                unsigned px = 0u;
                if (!blank) {
                    const int off = (int)((base0 + r * row_bytes) & 15) + 3 * (mirror ? W - 1 - x : x);
                    const unsigned* wp = raw32 + r * GS * 4 + (off >> 2);
                    const unsigned long long two = ((unsigned long long)wp[1] << 32) | wp[0];
                    px = (unsigned)(two >> (8 * (off & 3)));
                }
                o.x = lut[px & 255u]; o.y = lut[(px >> 8) & 255u]; o.z = lut[(px >> 16) & 255u];
            }
            mx = fmaxf(mx, fmaxf(m3t_fin_abs(o.x), fmaxf(m3t_fin_abs(o.y), m3t_fin_abs(o.z))));
            const long long pos = (long long)y * W + x;
            if (a.layout == 0) {
                *reinterpret_cast<float4*>(a.out + 4 * (nt * HW + pos)) = o;
            } else {
                float* q = a.out + ((long long)n * 3 * a.T + t) * HW + pos;
                const long long plane = (long long)a.T * HW;
                q[0] = o.x; q[plane] = o.y; q[2 * plane] = o.z;
            }
        }
    }
    if (a.slot) {                                            // (uniform; the table's LDS is free once every pick is done)
        __syncthreads();
        m3t_block_raise_slot(a.slot, mx, lut);
    }
}

// The reference's 256-pixel branch (dataset.py:61,73: crop 224, cv2.resize to 112 x 112): the window in the source is 2H x 2W and every
// output channel is the rounded mean of its 2 x 2 source block, (a + b + c + d + 2) >> 2 -- what OpenCV's resize computes for 8-bit images
// at an exact factor of 2 (its INTER_LINEAR takes the integer INTER_AREA path there).  The mean is a uint8 again, so the same table gather
// follows it.  Same design as above: one workgroup takes R output rows = 2R source row segments of 6 W bytes, staged from each segment's
// 16-byte floor; a pixel pair is 6 bytes at any byte offset, so a pick reads three dwords (the guard granule covers the last pair's third).
// LDS: 256 floats of table | 2R rows of (G + 1) granules
__global__ __launch_bounds__(256) void video_ingest_half_kernel(IngestArgs a) {
    extern __shared__ uint4 smem[];
    float* lut = reinterpret_cast<float*>(smem);
    uint4* raw = smem + 64;
    const unsigned* raw32 = reinterpret_cast<const unsigned*>(raw);
    const int tid = threadIdx.x, H = a.H, W = a.W, G = a.G, GS = a.G + 1;
    const long long HW = (long long)H * W;
    float mx = 0.f;
    for (long long unit = blockIdx.x; unit < a.units; unit += gridDim.x) {
        const long long nt = unit / a.tiles;
        const int tile = (int)(unit - nt * a.tiles);
        const int n = (int)(nt / a.T), t = (int)(nt - (long long)n * a.T);
        const int y0 = tile * a.R, rows = min(a.R, H - y0);
        const int* g = a.geom + 8 * (long long)n;
        // a bad device-side table cannot leave the allocation: window and frame index are clamped into range
        const int cy = min(max(g[0], 0), a.Hs - 2 * H), cx = min(max(g[1], 0), a.Ws - 2 * W), mirror = g[2];
        const int ky1 = g[3], ky2 = g[4], kx1 = g[5], kx2 = g[6];
        int f = a.frame_idx ? a.frame_idx[(long long)n * a.T + t] : t;
        const bool blank = f < 0;
        f = min(max(f, 0), a.Ts - 1);
        const long long row_bytes = 3ll * a.Ws;
        const long long base0 = ((((long long)n * a.Ts + f) * a.Hs + cy + 2 * y0) * a.Ws + cx) * 3;  // first byte of the tile's first source row segment
        __syncthreads();                                     // (the previous unit's picks are done)
        lut[tid] = a.lut[(long long)n * a.lut_stride + tid];
        if (!blank) {
            for (int i = tid; i < 2 * rows * G; i += 256) {
                const int r = i / G, q = i - r * G;          // r: source row of the tile, 0 .. 2 rows - 1
                const long long b = base0 + r * row_bytes, o = (b & ~15ll) + 16ll * q;
                if (o >= b + 6ll * W) continue;              // (a granule past the segment: never picked from)
                uint4 v;
                if (o + 16 <= a.bytes) {
                    v = *reinterpret_cast<const uint4*>(a.frames + o);
                } else {                                     // the allocation's last, partial granule: byte by byte
                    unsigned w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
                    for (int k = 0; k < 16; ++k)
                        if (o + k < a.bytes) w[k >> 2] |= (unsigned)a.frames[o + k] << (8 * (k & 3));
                    v = make_uint4(w[0], w[1], w[2], w[3]);
                }
                raw[r * GS + q] = v;
            }
        }
        __syncthreads();
        for (int p = tid; p < rows * W; p += 256) {
            const int r = p / W, x = p - r * W, y = y0 + r;
            float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!(y >= ky1 && y < ky2 && x >= kx1 && x < kx2)) {
                unsigned s0 = 0u, s1 = 0u, s2 = 0u;          // channel sums of the 2 x 2 block
                if (!blank) {
                    const int xs = mirror ? W - 1 - x : x;
#pragma unroll
                    for (int k = 0; k < 2; ++k) {
                        const int off = (int)((base0 + (2 * r + k) * row_bytes) & 15) + 6 * xs;
                        const unsigned* wp = raw32 + (2 * r + k) * GS * 4 + (off >> 2);
                        const unsigned w0 = wp[0], w1 = wp[1], w2 = wp[2];
                        const int sh = 8 * (off & 3);
                        const unsigned lo = (unsigned)((((unsigned long long)w1 << 32) | w0) >> sh);     // bytes 0..3 of the pair
                        const unsigned hi = (unsigned)((((unsigned long long)w2 << 32) | w1) >> sh);     // bytes 4..7
                        s0 += (lo & 255u) + (lo >> 24);
                        s1 += ((lo >> 8) & 255u) + (hi & 255u);
                        s2 += ((lo >> 16) & 255u) + ((hi >> 8) & 255u);
                    }
                }
                o.x = lut[(s0 + 2u) >> 2]; o.y = lut[(s1 + 2u) >> 2]; o.z = lut[(s2 + 2u) >> 2];
            }
            mx = fmaxf(mx, fmaxf(m3t_fin_abs(o.x), fmaxf(m3t_fin_abs(o.y), m3t_fin_abs(o.z))));
            const long long pos = (long long)y * W + x;
            if (a.layout == 0) {
                *reinterpret_cast<float4*>(a.out + 4 * (nt * HW + pos)) = o;
            } else {
                float* q = a.out + ((long long)n * 3 * a.T + t) * HW + pos;
                const long long plane = (long long)a.T * HW;
                q[0] = o.x; q[plane] = o.y; q[2 * plane] = o.z;
            }
        }
    }
    if (a.slot) {                                            // (uniform; the table's LDS is free once every pick is done)
        __syncthreads();
        m3t_block_raise_slot(a.slot, mx, lut);
    }
}

}  // namespace

extern "C" int m3t_video_ingest(const uint8_t* frames, int N, int Ts, int Hs, int Ws, const int* frame_idx, int T, const int* geom,
                                const float* lut, int lut_stride, int H, int W, int layout, float* out, void* stream) {
    unsigned long long* amax = m3t_take_amax_out();
    if (N < 0 || T < 0) return M3T_EINVAL;
    if (N == 0 || T == 0) return 0;
    if (!frames || !geom || !lut || !out || Ts <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || H > Hs || W > Ws ||
        (lut_stride != 0 && lut_stride != 256) || (layout != 0 && layout != 1) || (!frame_idx && T > Ts))
        return M3T_EINVAL;
    if (((uintptr_t)frames % 16) != 0 || ((uintptr_t)out % 16) != 0 || ((uintptr_t)geom % 4) != 0 || ((uintptr_t)lut % 4) != 0 ||
        ((uintptr_t)frame_idx % 4) != 0)
        return M3T_EINVAL;
    IngestArgs a;
    a.frames = frames; a.frame_idx = frame_idx; a.geom = geom; a.lut = lut; a.out = out; a.slot = amax;
    a.bytes = (long long)N * Ts * Hs * Ws * 3;
    a.Ts = Ts; a.Hs = Hs; a.Ws = Ws; a.T = T; a.H = H; a.W = W; a.lut_stride = lut_stride; a.layout = layout;
    a.G = (int)((15ll + 3ll * W + 15) / 16);                 // granules of a segment that starts at byte 15 of its first one
    int R = H < 16 ? H : 16;
    while (R > 1 && (size_t)R * (a.G + 1) * 16 > (48u << 10)) R >>= 1;
    const size_t lds = 1024 + (size_t)R * (a.G + 1) * 16;
    if (lds > (60u << 10)) return M3T_EINVAL;               // (rows wider than ~1000 pixels)
    a.R = R;
    a.tiles = (H + R - 1) / R;
    a.units = (long long)N * T * a.tiles;
    const long long blocks = a.units < 16384 ? a.units : 16384;
    video_ingest_kernel<<<(unsigned)blocks, 256, lds, (hipStream_t)stream>>>(a);
    M3T_LAUNCH_CHECK();
    return 0;
}

extern "C" int m3t_video_ingest_half(const uint8_t* frames, int N, int Ts, int Hs, int Ws, const int* frame_idx, int T, const int* geom,
                                     const float* lut, int lut_stride, int H, int W, int layout, float* out, void* stream) {
    unsigned long long* amax = m3t_take_amax_out();
    if (N < 0 || T < 0) return M3T_EINVAL;
    if (N == 0 || T == 0) return 0;
    if (!frames || !geom || !lut || !out || Ts <= 0 || Hs <= 0 || Ws <= 0 || H <= 0 || W <= 0 || 2ll * H > Hs || 2ll * W > Ws ||
        (lut_stride != 0 && lut_stride != 256) || (layout != 0 && layout != 1) || (!frame_idx && T > Ts))
        return M3T_EINVAL;
    if (((uintptr_t)frames % 16) != 0 || ((uintptr_t)out % 16) != 0 || ((uintptr_t)geom % 4) != 0 || ((uintptr_t)lut % 4) != 0 ||
        ((uintptr_t)frame_idx % 4) != 0)
        return M3T_EINVAL;
    IngestArgs a;
    a.frames = frames; a.frame_idx = frame_idx; a.geom = geom; a.lut = lut; a.out = out; a.slot = amax;
    a.bytes = (long long)N * Ts * Hs * Ws * 3;
    a.Ts = Ts; a.Hs = Hs; a.Ws = Ws; a.T = T; a.H = H; a.W = W; a.lut_stride = lut_stride; a.layout = layout;
    a.G = (int)((15ll + 6ll * W + 15) / 16);                 // granules of a source segment that starts at byte 15 of its first one
    int R = H < 16 ? H : 16;
    while (R > 1 && (size_t)2 * R * (a.G + 1) * 16 > (48u << 10)) R >>= 1;
    const size_t lds = 1024 + (size_t)2 * R * (a.G + 1) * 16;
    if (lds > (60u << 10)) return M3T_EINVAL;               // (output rows wider than ~5000 pixels)
    a.R = R;
    a.tiles = (H + R - 1) / R;
    a.units = (long long)N * T * a.tiles;
    const long long blocks = a.units < 16384 ? a.units : 16384;
    video_ingest_half_kernel<<<(unsigned)blocks, 256, lds, (hipStream_t)stream>>>(a);
    M3T_LAUNCH_CHECK();
    return 0;
}
