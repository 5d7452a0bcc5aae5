// csrc/cls_eval_core.h on the host: the schedule of cls_eval_rank_kernel (csrc/cls_eval.hip) with a loop over `tid` where the kernel has a
// workgroup barrier, on exact-size heap blocks (a sanitizer build sees every index), against a direct restatement: std::sort on
// (value, label) and a serial walk with 128-bit / long double arithmetic.
//   usage: cls_eval_host_check            runs the built-in cases (sizes x thread counts x LDS chunk lengths x tie patterns); exit 0: all agree
// The AUC numerator, P and the sorted keys must agree exactly; AP to (P + 2) 2^-52.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "cls_eval_core.h"

namespace {

struct Out { double ap; uint64_t num; unsigned P; };

uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

// the kernel's schedule: L items of "LDS", a "global" workspace when the padded column is longer, nt threads
Out emulate(const std::vector<float>& s, const std::vector<unsigned char>& l, unsigned nt, unsigned lds_rows) {
    const unsigned M = (unsigned)s.size(), n2 = (unsigned)cls_ceil_pow2(M), L = cls_floor_pow2(lds_rows);
    const unsigned Lu = n2 <= L ? n2 : L;
    std::vector<uint64_t> lds(Lu), ws(n2 <= L ? 0 : n2), bufA(nt), bufB(nt);
    auto load = [&](unsigned g0, unsigned n) { for (unsigned i = 0; i < n; ++i) lds[i] = g0 + i < M ? cls_item(bits_of(s[g0 + i]), l[g0 + i]) : 0ull; };
    auto step_lds = [&](unsigned n, unsigned g0, unsigned k, unsigned j) { for (unsigned t = 0; t < nt; ++t) cls_bitonic_step(lds.data(), n, g0, k, j, t, nt); };
    const uint64_t* sorted;
    if (n2 <= L) {
        load(0, n2);
        for (unsigned k = 2; k <= n2; k <<= 1)
            for (unsigned j = k >> 1; j > 0; j >>= 1) step_lds(n2, 0, k, j);
        sorted = lds.data();
    } else {
        for (unsigned g0 = 0; g0 < n2; g0 += L) {
            load(g0, L);
            for (unsigned k = 2; k <= L; k <<= 1)
                for (unsigned j = k >> 1; j > 0; j >>= 1) step_lds(L, g0, k, j);
            for (unsigned i = 0; i < L; ++i) ws[g0 + i] = lds[i];
        }
        for (unsigned k = 2 * L; k <= n2; k <<= 1) {
            for (unsigned j = k >> 1; j >= L; j >>= 1)
                for (unsigned t = 0; t < nt; ++t) cls_bitonic_step(ws.data(), n2, 0u, k, j, t, nt);
            for (unsigned g0 = 0; g0 < n2; g0 += L) {
                for (unsigned i = 0; i < L; ++i) lds[i] = ws[g0 + i];
                for (unsigned j = L >> 1; j > 0; j >>= 1) step_lds(L, g0, k, j);
                for (unsigned i = 0; i < L; ++i) ws[g0 + i] = lds[i];
            }
        }
        sorted = ws.data();
    }
    for (unsigned i = 0; i + 1 < n2; ++i)
        if (sorted[i] < sorted[i + 1]) { fprintf(stderr, "not sorted at %u (M %u, L %u)\n", i, M, L); exit(2); }
    std::vector<unsigned> cnt(nt), oi(nt), oc(nt), base(nt);
    std::vector<uint64_t> carry(nt);
    for (unsigned t = 0; t < nt; ++t) cls_walk_count(sorted, M, t, nt, cnt[t], oi[t], oc[t]);
    auto scan = [&](bool take_max) {
        uint64_t *src = bufA.data(), *dst = bufB.data();
        for (unsigned d = 1; d < nt; d <<= 1) {
            for (unsigned t = 0; t < nt; ++t) cls_scan_step(src, dst, d, t, take_max);
            std::swap(src, dst);
        }
        return src;
    };
    for (unsigned t = 0; t < nt; ++t) bufA[t] = cnt[t];
    uint64_t* r = scan(false);
    for (unsigned t = 0; t < nt; ++t) base[t] = t ? (unsigned)r[t - 1] : 0u;
    const unsigned P = (unsigned)r[nt - 1];
    for (unsigned t = 0; t < nt; ++t) bufA[t] = cls_open_word(oi[t], oc[t], base[t]);
    r = scan(true);
    for (unsigned t = 0; t < nt; ++t) carry[t] = t ? r[t - 1] : 0ull;
    std::vector<double> red(nt);
    std::vector<uint64_t> nums(nt);
    for (unsigned t = 0; t < nt; ++t) cls_walk_score(sorted, M, t, nt, base[t], carry[t], red[t], nums[t]);
    for (unsigned st = nt >> 1; st > 0; st >>= 1)
        for (unsigned t = 0; t < st; ++t) { red[t] += red[t + st]; nums[t] += nums[t + st]; }
    return Out{red[0], nums[0], P};
}

// the direct restatement: groups of equal VALUES (== on floats: -0.0 equals +0.0, denormals differ)
void direct(const std::vector<float>& s, const std::vector<unsigned char>& l, long double& ap, uint64_t& num, unsigned& P) {
    std::vector<unsigned> idx(s.size());
    for (unsigned i = 0; i < idx.size(); ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](unsigned a, unsigned b) { return s[a] > s[b]; });
    ap = 0; num = 0;
    uint64_t tp = 0, fp = 0;
    for (size_t a = 0; a < idx.size();) {
        size_t b = a;
        uint64_t dtp = 0, dfp = 0;
        while (b < idx.size() && s[idx[b]] == s[idx[a]]) { (l[idx[b]] ? dtp : dfp) += 1; ++b; }
        num += dfp * (2 * tp + dtp);
        tp += dtp; fp += dfp;
        ap += (long double)dtp * (long double)tp / (long double)(tp + fp);
        a = b;
    }
    P = (unsigned)tp;
}

unsigned long long rng = 0x9E3779B97F4A7C15ull;
unsigned next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (unsigned)(rng >> 32); }

}  // namespace

int main() {
    const unsigned sizes[] = {1, 2, 3, 7, 63, 64, 65, 257, 1000, 4097};
    const unsigned threads[] = {1, 8, 64, 1024};
    const unsigned chunks[] = {1, 2, 16, 100, 1024, 16384};
    int cases = 0;
    for (unsigned M : sizes)
        for (int pattern = 0; pattern < 6; ++pattern) {
            std::vector<float> s(M);
            std::vector<unsigned char> l(M);
            for (unsigned i = 0; i < M; ++i) {
                const unsigned r = next();
                switch (pattern) {
                    case 0: s[i] = (float)(int)(r % 2000001u) * 1e-3f - 1000.f; break;          // (nearly) untied
                    case 1: s[i] = (float)(r % 4u) - 1.5f; break;                             // 4 values
                    case 2: s[i] = 0.25f; break;                                              // one group
                    case 3: s[i] = (r & 1u) ? -0.0f : 0.0f; if (r % 5u == 0) s[i] = 1.f; break;   // both zeros tie
                    case 4: s[i] = (r & 1u) ? 1e-40f : 2e-40f; if (r % 7u == 0) s[i] = -1e-40f; break;   // denormals differ
                    default: s[i] = (float)(i / 37u); break;                                  // long runs across chunk boundaries
                }
                l[i] = (unsigned char)(next() % 3u == 0);
            }
            long double ap_ref; uint64_t num_ref; unsigned P_ref;
            direct(s, l, ap_ref, num_ref, P_ref);
            for (unsigned nt : threads)
                for (unsigned L : chunks) {
                    const Out o = emulate(s, l, nt, L);
                    ++cases;
                    if (o.P != P_ref || o.num != num_ref || fabsl((long double)o.ap - ap_ref) > (long double)(P_ref + 2) * ldexpl(1.0L, -52) * (P_ref ? P_ref : 1)) {
                        fprintf(stderr, "M %u pattern %d nt %u L %u: P %u / %u, num %llu / %llu, ap sum %.17g / %.17Lg\n", M, pattern, nt, L, o.P,
                                P_ref, (unsigned long long)o.num, (unsigned long long)num_ref, o.ap, ap_ref);
                        return 3;
                    }
                }
        }
    printf("cls_eval_host_check: %d cases agree\n", cases);
    return 0;
}
