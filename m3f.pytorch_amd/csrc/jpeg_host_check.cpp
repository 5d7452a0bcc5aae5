// The device code of csrc/jpeg.hip on the host: this program includes jpeg_core.h, reads one packed batch (the arguments of
// m3t_jpeg_decode as m3t.jpeg.pack builds them) from a file, decodes it with the schedule of the two kernels run sequentially, and
// writes status and pixels to a second file.  tests/test_jpeg_host.py builds it with the host compiler and compares the result with the
// goldens; built with -fsanitize=address,undefined it is the memory check of the decoder's text (as a plain executable).
//   input : int32 header[12] = magic, n, n_segs, n_quant, n_huff, H, W, order, dst_slots, stream_bytes, 0, 0 | tables | stream bytes
//   output: int32 status[n] | uint8 dst[dst_slots][H][W][3], every byte the decoder did not write still GUARD
// The stream, the workspace and the destination are separate exact-size heap blocks with guard bytes around the last two, which are
// checked before the program reports success.  Exit 0: decoded (whatever the status words say); 2: the tables were refused
// (M3T_EINVAL's rule); 3: a guard byte changed; 1: usage or I/O.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "jpeg_core.h"

static const unsigned char GUARD = 0xA5;
static const int GUARD_BYTES = 64;
static const uint8_t kZigzag[64] = JPEG_ZIGZAG_INIT;

static int decode_segment(const uint8_t* stream, long long stream_bytes, const int* t, int n, int n_segs, int n_quant, int H, int W, int s,
                          uint8_t* ws, long long slot_bytes) {
    const int* seg = t + (long long)n * JPEG_IMG_COLS + (long long)s * JPEG_SEG_COLS;
    const int* quant = t + (long long)n * JPEG_IMG_COLS + (long long)n_segs * JPEG_SEG_COLS + n;
    const int* huff = quant + (long long)n_quant * JPEG_QUANT_INTS;
    const int i = seg[0];
    const int* im = t + (long long)i * JPEG_IMG_COLS;
    const JpegGeom g = jpeg_geom(im, H, W);
    const int total = g.mcus_x * g.mcus_y, Ri = im[4], k = s - im[5];
    const int m0 = k * Ri, m1 = m0 + Ri < total ? m0 + Ri : total;
    uint8_t* planes = ws + slot_bytes * i;
    JpegReader r;
    jpeg_reader_init(r, stream, 0, (int)stream_bytes, seg[1], seg[1] + seg[2]);
    int pred[3] = {0, 0, 0};
    bool dead = false;
    for (int m = m0; m < m1; ++m) {
        int16_t coef[6 * 64];
        int32_t wsp[6 * 64];
        memset(coef, 0, sizeof(coef));
        for (int b = 0; b < g.blocks && !dead; ++b) {
            int comp, y0, x0;
            jpeg_block_place(g, m, b, comp, y0, x0);
            const JpegHuff hd = jpeg_huff_at(huff + (long long)JPEG_HUFF_INTS * im[10 + comp]);
            const JpegHuff ha = jpeg_huff_at(huff + (long long)JPEG_HUFF_INTS * im[13 + comp]);
            const int st = jpeg_decode_block(r, hd, ha, kZigzag, pred[comp], coef + 64 * b, true);
            if (st) { r.status |= st; dead = true; }
        }
        for (int b = 0; b < g.blocks; ++b) {
            int comp, y0, x0;
            jpeg_block_place(g, m, b, comp, y0, x0);
            const uint16_t* q = reinterpret_cast<const uint16_t*>(quant + (long long)JPEG_QUANT_INTS * im[7 + comp]);
            for (int x = 0; x < 8; ++x) jpeg_idct_col(coef + 64 * b, q, x, wsp + 64 * b);
            for (int y = 0; y < 8; ++y) {
                uint32_t w[2];
                jpeg_idct_row(wsp + 64 * b, y, w[0], w[1]);
                uint8_t* o = planes + g.plane[comp] + (long long)(y0 + y) * g.stride[comp] + x0;
                for (int x = 0; x < 8; ++x) o[x] = (uint8_t)(w[x >> 2] >> (8 * (x & 3)));
            }
        }
    }
    int st = r.status | (dead ? 0 : jpeg_segment_tail(r));
    if (k > 0 && seg[3] != ((k - 1) & 7)) st |= JPEG_ST_RST;
    if (im[0] & 2) st |= JPEG_ST_RST;
    return st;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s packed.bin out.bin\n", argv[0]); return 1; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 1; }
    int hd[12];
    if (fread(hd, 4, 12, f) != 12 || hd[0] != 0x4A504731) { fprintf(stderr, "bad header\n"); return 1; }
    const int n = hd[1], n_segs = hd[2], n_quant = hd[3], n_huff = hd[4], H = hd[5], W = hd[6], order = hd[7];
    const long long dst_slots = hd[8], stream_bytes = hd[9];
    if (n <= 0 || n > (1 << 20) || n_segs < 0 || n_segs > (1 << 24) || n_quant < 0 || n_quant > 4096 || n_huff < 0 || n_huff > 4096 || stream_bytes < 0) {
        fprintf(stderr, "tables refused\n");
        return 2;
    }
    std::vector<int> t((size_t)jpeg_tables_ints(n, n_segs, n_quant, n_huff));
    if (fread(t.data(), 4, t.size(), f) != t.size()) { fprintf(stderr, "short tables\n"); return 1; }
    uint8_t* stream = (uint8_t*)malloc(stream_bytes ? (size_t)stream_bytes : 1);          // exact size: a read past it is the sanitizer's to see
    if (stream_bytes && fread(stream, 1, (size_t)stream_bytes, f) != (size_t)stream_bytes) { fprintf(stderr, "short stream\n"); return 1; }
    fclose(f);
    if (!jpeg_tables_ok(t.data(), n, n_segs, n_quant, n_huff, H, W, stream_bytes, dst_slots)) { fprintf(stderr, "tables refused\n"); return 2; }

    const long long slot_bytes = jpeg_slot_bytes(H, W), ws_bytes = slot_bytes * n, frame = 3ll * H * W, dst_bytes = frame * dst_slots;
    uint8_t* ws_block = (uint8_t*)malloc((size_t)ws_bytes + 2 * GUARD_BYTES);
    uint8_t* dst_block = (uint8_t*)malloc((size_t)dst_bytes + 2 * GUARD_BYTES);
    memset(ws_block, GUARD, (size_t)ws_bytes + 2 * GUARD_BYTES);
    memset(dst_block, GUARD, (size_t)dst_bytes + 2 * GUARD_BYTES);
    uint8_t* ws = ws_block + GUARD_BYTES;
    uint8_t* dst = dst_block + GUARD_BYTES;
    std::vector<int> status((size_t)n, 0);
    const int* slot = t.data() + (long long)n * JPEG_IMG_COLS + (long long)n_segs * JPEG_SEG_COLS;

    for (int s = 0; s < n_segs; ++s) {
        const int i = t[(size_t)n * JPEG_IMG_COLS + (size_t)s * JPEG_SEG_COLS];
        status[i] |= decode_segment(stream, stream_bytes, t.data(), n, n_segs, n_quant, H, W, s, ws, slot_bytes);
    }
    for (int i = 0; i < n; ++i) {
        const int* im = t.data() + (long long)i * JPEG_IMG_COLS;
        uint8_t* o = dst + frame * slot[i];
        if (!(im[0] & 1)) { memset(o, 0, (size_t)frame); continue; }
        const JpegGeom g = jpeg_geom(im, H, W);
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x, o += 3) {
                const uint32_t p = jpeg_pixel(ws + slot_bytes * i, g, y, x);
                o[order ? 0 : 2] = (uint8_t)p; o[1] = (uint8_t)(p >> 8); o[order ? 2 : 0] = (uint8_t)(p >> 16);
            }
    }
    int bad = 0;
    for (int j = 0; j < GUARD_BYTES; ++j)
        bad |= ws_block[j] != GUARD || ws_block[GUARD_BYTES + ws_bytes + j] != GUARD || dst_block[j] != GUARD || dst_block[GUARD_BYTES + dst_bytes + j] != GUARD;
    if (bad) { fprintf(stderr, "a guard byte changed\n"); return 3; }
    f = fopen(argv[2], "wb");
    if (!f) { perror(argv[2]); return 1; }
    fwrite(status.data(), 4, (size_t)n, f);
    fwrite(dst, 1, (size_t)dst_bytes, f);
    fclose(f);
    free(stream); free(ws_block); free(dst_block);
    int nz = 0;
    for (int i = 0; i < n; ++i) nz += status[i] != 0;
    printf("decoded %d images, %d with a non-zero status\n", n, nz);
    return 0;
}
