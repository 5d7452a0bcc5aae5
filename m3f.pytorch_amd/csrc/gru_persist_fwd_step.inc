// One step of gru_persist_fwd_kernel (included twice: even steps use the x-projection registers A and request B, odd
// steps the reverse).  STEPV = the step index, CUR(x) / NXT(x) = the register set in use / being filled.
    {
        const int step = STEPV;
        const int t = d.reverse ? T - 1 - step : step;
        M3T_STAMP(0);
        if (step > 0) {
            const unsigned tag = ex.tag_base + (unsigned)step;       // h_{step-1} carries tag (step-1)+1
            const unsigned long long* src = gran + (size_t)((step - 1) & 1) * slot + grp + (size_t)wave * TILE + lane;
            unsigned long long v[NC][RT][4];
            int spins = 0;
            M3T_GATHER_DELAY(step);
            for (;;) {
#pragma unroll
                for (int m = 0; m < NC; ++m)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {          // one address per (chunk, row tile); e by immediate offset
                        const unsigned long long* q = src + (size_t)m * NW * TILE + rt * 256;
                        asm volatile("global_load_dwordx2 %0, %4, off sc1\n\t"
                                     "global_load_dwordx2 %1, %4, off offset:512 sc1\n\t"
                                     "global_load_dwordx2 %2, %4, off offset:1024 sc1\n\t"
                                     "global_load_dwordx2 %3, %4, off offset:1536 sc1"
                                     : "=&v"(v[m][rt][0]), "=&v"(v[m][rt][1]), "=&v"(v[m][rt][2]), "=&v"(v[m][rt][3])
                                     : "v"(q) : "memory");
                    }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bool ok = true;
#pragma unroll
                for (int m = 0; m < NC; ++m)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            asm volatile("" : "+v"(v[m][rt][e]));          // defined only after the wait above
                            ok = ok && ((unsigned)(v[m][rt][e] >> 32) == tag);
                        }
                M3T_GATHER_RETRY(ok, step);
            }
            gather_note_fail(spins, lane, &poll_fail[step & 1]);
            M3T_STAMP(1);
            f32x4 acc[RT][3];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < 3; ++ct) acc[rt][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int m = 0; m < NC; ++m)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                    for (int ct = 0; ct < 3; ++ct) {
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float((unsigned)v[m][rt][0]), wf[m][ct].x, acc[rt][ct], 0, 0, 0);
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float((unsigned)v[m][rt][1]), wf[m][ct].y, acc[rt][ct], 0, 0, 0);
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float((unsigned)v[m][rt][2]), wf[m][ct].z, acc[rt][ct], 0, 0, 0);
                        acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float((unsigned)v[m][rt][3]), wf[m][ct].w, acc[rt][ct], 0, 0, 0);
                    }
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                for (int ct = 0; ct < 3; ++ct)
#pragma unroll
                    for (int r = 0; r < 4; ++r) red[step & (NB - 1)][wave][ct][rt * 16 + (lane >> 4) * 4 + r][lane & 15] = acc[rt][ct][r];
        }
        cell_phase_wait();
        // every step, unconditionally (a conditional definition gets merged by copies that read registers in flight):
        // this step's x-projection (requested one step ago) is complete since the gather's vmcnt(0) (step 0: the
        // prologue's); with nothing else outstanding, request the next step's into the other register set
        asm volatile("" : "+v"(CUR(xr)), "+v"(CUR(xz)), "+v"(CUR(xn)));
        M3T_FWD_LOAD_X(step + 1, NXT(xr), NXT(xz), NXT(xn));
        M3T_STAMP(2);
        __syncthreads();
        M3T_POLL_ADAPT(step & 1, (step + 1) & 1, step);
        M3T_STAMP(3);
        if (pw) {
            float hr = br, hz = bz, hn = bn;
            if (step > 0) {
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    hr += red[step & (NB - 1)][w][0][prow][pu];
                    hz += red[step & (NB - 1)][w][1][prow][pu];
                    hn += red[step & (NB - 1)][w][2][prow][pu];
                }
            }
            const GateFwd c = gru_cell_fwd(CUR(xr), CUR(xz), CUR(xn), hr, hz, hn, hprev);
            if (M3T_SCAN_PUBLISHES(step, true)) {          // 8-byte granule {h, tag32}
                const unsigned long long gq = ((unsigned long long)(ex.tag_base + (unsigned)step + 1u) << 32) | __float_as_uint(pok ? (g.bf16 ? rbf(c.h) : c.h) : 0.f);
                M3T_PUBLISH8(gran + (size_t)(step & 1) * slot + pub, gq);
            }
            M3T_MARK_PUBLISHED(step);
            M3T_STAMP(4);
            hprev = c.h;
            if (pok) M3T_FWD_STORE_RESULTS(pb, pj, t, step == T - 1, float4, make_float4(c.r, c.z, c.n, hn), c.h);
        }
        if (NB == 1) __syncthreads();
        M3T_STAMP(5);
    }
