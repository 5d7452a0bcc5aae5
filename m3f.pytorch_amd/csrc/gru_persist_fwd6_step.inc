// One step of gru_persist_fwd6_kernel (included twice: even steps use the x-projection registers A and request B, odd
// steps the reverse).  STEPV = the step index, CUR(x) / NXT(x) = the register set in use / being filled.
    {
        const int step = STEPV;
        const int t = d.reverse ? T - 1 - step : step;
        M3T_STAMP(0);
        M3T_MARK_STEP_TOP(step);
        if (step > 0) {
            const unsigned tag = (ex.tag_base + (unsigned)step) & 0xffffu;
            const unsigned long long* src = gran + (size_t)(1 - PARV) * slot + grp + lane_off;
            pu32x4 v[KS][4];                               // [k-step][unit pair jp] = {lo(j0), hi(j0), lo(j1), hi(j1)}
            int spins = 0;
            M3T_GATHER_DELAY(step);
            for (;;) {
                // ONE 16-byte load takes two adjacent granules: the exchange is priced per load instruction, not per byte
                // (tools/persist_probe.hip: 8 dwordx4 instead of 16 dwordx2 loads = 1.63 vs 2.03 us per step)
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    const unsigned long long* qp = src + (size_t)(2 * k) * NW * TILE;
                    if (RB < ROWS)
                        // 8-clip row blocks: HALF the load instructions -- lane (r = lane & 7, hb = (lane >> 3) & 1) takes unit pair jp = hb
                        // and jp = 2 + hb of row r (lane_off8); the odd pairs move to the lanes of rows 0..7 behind the wait (DPP, below)
                        asm volatile("global_load_dwordx4 %0, %2, off sc1\n\t"
                                     "global_load_dwordx4 %1, %2, off offset:1024 sc1"
                                     : "=&v"(v[k][0]), "=&v"(v[k][2]) : "v"(qp) : "memory");
                    else
                    asm volatile("global_load_dwordx4 %0, %4, off sc1\n\t"
                                 "global_load_dwordx4 %1, %4, off offset:512 sc1\n\t"
                                 "global_load_dwordx4 %2, %4, off offset:1024 sc1\n\t"
                                 "global_load_dwordx4 %3, %4, off offset:1536 sc1"
                                 : "=&v"(v[k][0]), "=&v"(v[k][1]), "=&v"(v[k][2]), "=&v"(v[k][3])
                                 : "v"(qp) : "memory");
                }
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                bool ok = true;
#pragma unroll
                for (int k = 0; k < KS; ++k)
#pragma unroll
                    for (int jp = 0; jp < 4; jp += (RB < ROWS ? 2 : 1)) {
                        asm volatile("" : "+v"(v[k][jp]));
                        ok = ok && ((v[k][jp].y >> 16) == tag) && ((v[k][jp].w >> 16) == tag);
                    }
                M3T_GATHER_RETRY(ok, step);
            }
            gather_note_fail(spins, lane, &poll_fail[PARV]);
            M3T_STAMP(1);
            if (F16) {
                // fp16x3: granule = {fp16 hi, fp16 lo, 0, tag}; products lo hi, hi lo, hi hi.  The A operands of all k-steps first (the gather
                // registers die here), then one unit tile at a time (12 accumulator registers live instead of 24: the wide form with the
                // coalesced hand-over spilled into scratch -- vector-memory operations in front of the gather's wait -- without this)
                pf16x8 F1[KS], F2[KS];
                if (RB < ROWS) {
                    // the odd unit pairs sit in the lanes 8 up (same row r): rotate each row of 16 lanes by 8.  Lanes 8..15 of a row of 16
                    // end up with operand rows 8..15 that mean nothing -- and reach nothing: MFMA output row i reads operand row i only
#pragma unroll
                    for (int k = 0; k < KS; ++k)
#pragma unroll
                        for (int jp = 0; jp < 4; jp += 2) {
                            v[k][jp + 1].x = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v[k][jp].x, 0x128, 0xf, 0xf, false);      // row_ror:8
                            v[k][jp + 1].z = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v[k][jp].z, 0x128, 0xf, 0xf, false);
                        }
                }
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    pu32x4 a1, a2;
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        a1[jj] = __builtin_amdgcn_perm(v[k][jj].z, v[k][jj].x, 0x05040100u);
                        a2[jj] = __builtin_amdgcn_perm(v[k][jj].z, v[k][jj].x, 0x07060302u);
                    }
                    F1[k] = __builtin_bit_cast(pf16x8, a1); F2[k] = __builtin_bit_cast(pf16x8, a2);
                }
#pragma unroll
                for (int u = 0; u < UW; ++u) {             // (the A operand is shared by the workgroup's unit tiles)
                    f32x4 acc[3];
#pragma unroll
                    for (int ct = 0; ct < 3; ++ct) acc[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int k = 0; k < KS; ++k)
#pragma unroll
                        for (int ct = 0; ct < 3; ++ct) {
                            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F2[k], __builtin_bit_cast(pf16x8, wf[u][k][ct][0]), acc[ct], 0, 0, 0);
                            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F1[k], __builtin_bit_cast(pf16x8, wf[u][k][ct][1]), acc[ct], 0, 0, 0);
                            acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(F1[k], __builtin_bit_cast(pf16x8, wf[u][k][ct][0]), acc[ct], 0, 0, 0);
                        }
#pragma unroll
                    for (int ct = 0; ct < 3; ++ct)
#pragma unroll
                        for (int r = 0; r < 4; ++r) M3T_RED(PARV, wave, u, ct, (lane >> 4) * 4 + r, lane & 15) = acc[ct][r];
                }
            } else {
                f32x4 acc[UW][3];
#pragma unroll
                for (int u = 0; u < UW; ++u)
#pragma unroll
                    for (int ct = 0; ct < 3; ++ct) acc[u][ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < KS; ++k) {
                    pu32x4 a1, a2, a3;                     // the three terms of 8 consecutive units, paired into dwords
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj) {
                        a1[jj] = __builtin_amdgcn_perm(v[k][jj].z, v[k][jj].x, 0x05040100u);
                        a2[jj] = __builtin_amdgcn_perm(v[k][jj].z, v[k][jj].x, 0x07060302u);
                        a3[jj] = __builtin_amdgcn_perm(v[k][jj].w, v[k][jj].y, 0x05040100u);
                    }
                    const pbf16x8 A1 = __builtin_bit_cast(pbf16x8, a1), A2 = __builtin_bit_cast(pbf16x8, a2),
                                  A3 = __builtin_bit_cast(pbf16x8, a3);
#pragma unroll
                    for (int u = 0; u < UW; ++u)
#pragma unroll
                        for (int ct = 0; ct < 3; ++ct) {   // smallest terms first
                            acc[u][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A3, wf[u][k][ct][0], acc[u][ct], 0, 0, 0);
                            acc[u][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A2, wf[u][k][ct][1], acc[u][ct], 0, 0, 0);
                            acc[u][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A1, wf[u][k][ct][NTERM - 1], acc[u][ct], 0, 0, 0);
                            acc[u][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A2, wf[u][k][ct][0], acc[u][ct], 0, 0, 0);
                            acc[u][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A1, wf[u][k][ct][1], acc[u][ct], 0, 0, 0);
                            acc[u][ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A1, wf[u][k][ct][0], acc[u][ct], 0, 0, 0);
                        }
                }
#pragma unroll
                for (int u = 0; u < UW; ++u)
#pragma unroll
                    for (int ct = 0; ct < 3; ++ct)
#pragma unroll
                        for (int r = 0; r < 4; ++r) M3T_RED(PARV, wave, u, ct, (lane >> 4) * 4 + r, lane & 15) = acc[u][ct][r];
            }
        }
        cell_phase_wait();
        // every step, unconditionally (a conditional definition gets merged by copies that read registers in flight):
        // this step's x-projection (requested one step ago) is complete since the gather's vmcnt(0) (step 0: the
        // prologue's); with nothing else outstanding, request the next step's into the other register set
        asm volatile("" : "+v"(CUR(xr)), "+v"(CUR(xz)), "+v"(CUR(xn)));
        if (CO && pw) sx[PARV * UW * SLOTS + slot_h] = (f32x4){CUR(xr), CUR(xz), CUR(xn), 0.f};      // loaded in memory order: to its cell thread
        M3T_FWD_LOAD_X(step + 1, NXT(xr), NXT(xz), NXT(xn));
        M3T_STAMP(2);
        __syncthreads();
        M3T_MARK_AFTER_BARRIER(step);
        M3T_POLL_ADAPT(PARV, 1 - PARV, step);
        M3T_STAMP(3);
        if (pw) {
            float hr = br, hz = bz, hn = bn;
            if (step > 0) {
                if (F16) {                                 // the waves' sums carry the scales of h and of the W_hh slice
                    float sr = 0.f, sz = 0.f, sn = 0.f;
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        sr += M3T_RED(PARV, w, tu, 0, prow, pu);
                        sz += M3T_RED(PARV, w, tu, 1, prow, pu);
                        sn += M3T_RED(PARV, w, tu, 2, prow, pu);
                    }
                    hr = fmaf(sr, winv, br); hz = fmaf(sz, winv, bz); hn = fmaf(sn, winv, bn);
                } else {
#pragma unroll
                    for (int w = 0; w < NW; ++w) {
                        hr += M3T_RED(PARV, w, tu, 0, prow, pu);
                        hz += M3T_RED(PARV, w, tu, 1, prow, pu);
                        hn += M3T_RED(PARV, w, tu, 2, prow, pu);
                    }
                }
            }
            float c_xr = CUR(xr), c_xz = CUR(xz), c_xn = CUR(xn);
            if (CO) { const f32x4 x4 = sx[PARV * UW * SLOTS + slot_c]; c_xr = x4[0]; c_xz = x4[1]; c_xn = x4[2]; }
            const GateFwd c = gru_cell_fwd(c_xr, c_xz, c_xn, hr, hz, hn, hprev);
            if (M3T_SCAN_PUBLISHES(step, RB == ROWS || plive)) {      // (rows past an 8-clip block publish nothing)
                const float hv = pok ? (g.bf16 ? rbf(c.h) : c.h) : 0.f;
                unsigned long long gq;
                if (F16) {                                 // two fp16 terms of 2^14 h (|h| <= 1)
                    const float hs = hv * 16384.f;
                    const _Float16 f1 = (_Float16)hs;
                    const _Float16 f2 = (_Float16)(hs - (float)f1);
                    gq = (unsigned long long)__builtin_bit_cast(unsigned short, f1) |
                         ((unsigned long long)__builtin_bit_cast(unsigned short, f2) << 16) |
                         ((unsigned long long)((ex.tag_base + (unsigned)step + 1u) & 0xffffu) << 48);
                } else {
                    const __bf16 h1 = (__bf16)hv;
                    const float r1 = hv - (float)h1;
                    const __bf16 h2 = (__bf16)r1;
                    const __bf16 h3 = (__bf16)(r1 - (float)h2);
                    gq = (unsigned long long)__builtin_bit_cast(unsigned short, h1) |
                         ((unsigned long long)__builtin_bit_cast(unsigned short, h2) << 16) |
                         ((unsigned long long)__builtin_bit_cast(unsigned short, h3) << 32) |
                         ((unsigned long long)((ex.tag_base + (unsigned)step + 1u) & 0xffffu) << 48);
                }
                M3T_PUBLISH8(gran + (size_t)PARV * slot + pub, gq);
            }
            M3T_MARK_PUBLISHED(step);
            M3T_STAMP(4);
            hprev = c.h;
            if (CO) {
                // results to LDS; the memory-order thread stores the PREVIOUS step's (written before this step's barrier)
                so[PARV * UW * SLOTS + slot_c] = (f32x4){c.r, c.z, c.n, hn};
                sh[PARV * UW * SLOTS + slot_c] = c.h;
                if (step > 0 && hok) store_results(step - 1, so[(1 - PARV) * UW * SLOTS + slot_h], sh[(1 - PARV) * UW * SLOTS + slot_h]);
            } else if (pok) {
                M3T_FWD_STORE_RESULTS(pb, pj, t, step == T - 1, float4, make_float4(c.r, c.z, c.n, hn), c.h);
            }
        }
        M3T_STAMP(5);
    }
