// One step of gru_persist_bwd3q_kernel: the wide producer-split backward scan with 32-deep MFMAs over PAIRS of producer tiles (a wide
// workgroup publishes two adjacent 16-unit tiles under ONE scale, so a consumer's v_mfma_f32_16x16x32_f16 may span both: half the
// MFMAs of the 16-deep form).  Included twice: even steps read the activation set A and request B, odd steps the reverse.
// STEPV = the step index, PARV = its parity (compile-time 0 / 1), CUR(x) / NXT(x) = the register set in use / being filled.
{
    const int step = STEPV;
    const bool has_next = step > 0;
    M3T_QSTAMP(0);
    M3T_MARK_STEP_TOP(step);
    if (has_next) {
        const unsigned tag = (ex.tag_base + (unsigned)step) & 0xffffffu;
        const u32x4* src = gran + (size_t)(1 - PARV) * slot + grp + lane_src;
        u32x4 v[NP][8];                                // [pair of this wave's K-slice][unit e of this lane's 8]: {hi|lo dr, hi|lo dz, hi|lo dnr, tag24|exp}
        int spins = 0;
        M3T_POLL_SLEEP();                              // (M3T_GATHER_DELAY without the wait for pub_step: no wave of this kernel arrives early)
        for (;;) {
#pragma unroll
            for (int m = 0; m < NP; ++m) {
                const u32x4* q = src + (size_t)m * NW * 2 * TILE;
                if (RB < ROWS)
                    // 8-clip row blocks: HALF the load instructions -- lane (r = lane & 7, hb = (lane >> 3) & 1) takes the units e = 2 i + hb
                    // of row r (lane_src); the odd units move to the lanes of rows 0..7 behind the wait (DPP, below)
                    asm volatile("global_load_dwordx4 %0, %4, off sc1\n\t"
                                 "global_load_dwordx4 %1, %4, off offset:1024 sc1\n\t"
                                 "global_load_dwordx4 %2, %4, off offset:2048 sc1\n\t"
                                 "global_load_dwordx4 %3, %4, off offset:3072 sc1"
                                 : "=&v"(v[m][0]), "=&v"(v[m][2]), "=&v"(v[m][4]), "=&v"(v[m][6]) : "v"(q) : "memory");
                else
                asm volatile("global_load_dwordx4 %0, %8, off sc1\n\t"
                             "global_load_dwordx4 %1, %8, off offset:512 sc1\n\t"
                             "global_load_dwordx4 %2, %8, off offset:1024 sc1\n\t"
                             "global_load_dwordx4 %3, %8, off offset:1536 sc1\n\t"
                             "global_load_dwordx4 %4, %8, off offset:2048 sc1\n\t"
                             "global_load_dwordx4 %5, %8, off offset:2560 sc1\n\t"
                             "global_load_dwordx4 %6, %8, off offset:3072 sc1\n\t"
                             "global_load_dwordx4 %7, %8, off offset:3584 sc1"
                             : "=&v"(v[m][0]), "=&v"(v[m][1]), "=&v"(v[m][2]), "=&v"(v[m][3]),
                               "=&v"(v[m][4]), "=&v"(v[m][5]), "=&v"(v[m][6]), "=&v"(v[m][7])
                             : "v"(q) : "memory");
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            bool ok = true;
#pragma unroll
            for (int m = 0; m < NP; ++m)
#pragma unroll
                for (int e = 0; e < 8; e += (RB < ROWS ? 2 : 1)) {
                    asm volatile("" : "+v"(v[m][e]));              // defined only after the wait above
                    ok = ok && ((v[m][e].w & 0xffffffu) == tag);
                }
            M3T_GATHER_RETRY(ok, step);
        }
        gather_note_fail(spins, lane, &poll_fail[PARV]);
        M3T_QSTAMP(1);
        // per pair m: this lane holds the granules of its 8 consecutive k (units 8 (q&1) + e of tile q>>1): dword g of a granule =
        // (hi | lo << 16) of gate g -- four v_perm pack the eight hi (lo) terms into the A operand of a 32-deep fp16 MFMA; three MFMAs per
        // gate (lo hi, hi lo, hi hi) accumulate the pair's partial product, which leaves its producer's scale on the way into the sum
        f32x4 acc[2];
        acc[0] = acc[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int m = 0; m < NP; ++m) {
            if (RB < ROWS) {
                // the odd units sit in the lanes 8 up (same row r): rotate each row of 16 lanes by 8.  Lanes 8..15 of a row of 16 end up with
                // operand rows 8..15 that mean nothing -- and reach nothing: MFMA output row i reads operand row i only
#pragma unroll
                for (int e = 0; e < 8; e += 2)
#pragma unroll
                    for (int gt = 0; gt < 3; ++gt)
                        v[m][e + 1][gt] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)v[m][e][gt], 0x128, 0xf, 0xf, false);      // row_ror:8
            }
            f32x4 at[2];
            at[0] = at[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int gt = 0; gt < 3; ++gt) {
                pu32x4 ah, al;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    ah[i] = __builtin_amdgcn_perm(v[m][2 * i + 1][gt], v[m][2 * i][gt], 0x05040100u);
                    al[i] = __builtin_amdgcn_perm(v[m][2 * i + 1][gt], v[m][2 * i][gt], 0x07060302u);
                }
                const pf16x8 AH = __builtin_bit_cast(pf16x8, ah), AL = __builtin_bit_cast(pf16x8, al);
#pragma unroll
                for (int u = 0; u < 2; ++u) {              // (the A operand is shared by the workgroup's two unit tiles)
                    at[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AL, __builtin_bit_cast(pf16x8, wb[u][gt][m][0]), at[u], 0, 0, 0);
                    at[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AH, __builtin_bit_cast(pf16x8, wb[u][gt][m][1]), at[u], 0, 0, 0);
                    at[u] = __builtin_amdgcn_mfma_f32_16x16x32_f16(AH, __builtin_bit_cast(pf16x8, wb[u][gt][m][0]), at[u], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);         // keep the packing of the next gate's operands behind these MFMAs (register pressure: the kernel sits at 256 VGPRs)
            }
            const float pinv = __uint_as_float((254u - (v[m][0].w >> 24)) << 23);       // 1 / (the producer workgroup's scale)
#pragma unroll
            for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[u][r] = fmaf(at[u][r], pinv, acc[u][r]);
        }
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[PARV][wave][u][(lane >> 4) * 4 + r][lane & 15] = acc[u][r] * winv[u];
    }
    cell_phase_wait();
    // this step's activations (requested one step ago), loaded in memory order: to the cell threads through LDS.  ONE place, behind the
    // unconditional wait: defined on two paths (inside and outside the gather branch) hipcc merged them with copies that read the
    // registers while the loads were still in flight (tools/check_inflight.py caught it)
    asm volatile("" : "+v"(CUR(dout)), "+v"(CUR(g4)), "+v"(CUR(hprev)));
    sin4[PARV * 2 * SLOTS + slot_h] = CUR(g4);
    sin2[PARV * 2 * SLOTS + slot_h] = make_float2(CUR(dout), CUR(hprev));
    // every step, unconditionally (a conditional definition gets merged by copies that read registers in flight): with
    // nothing else outstanding, request the next step's activations -- a whole step to arrive
    M3T_BWD_LOAD_STEP(step + 1, NXT(dout), NXT(g4), NXT(hprev));
    M3T_QSTAMP(2);
    __syncthreads();
    M3T_MARK_AFTER_BARRIER(step);
    M3T_POLL_ADAPT(PARV, 1 - PARV, step);
    M3T_QSTAMP(3);
    {
        float mm = 0.f;
        if (has_next) {
#pragma unroll
            for (int w = 0; w < NW; ++w) mm += red[PARV][w][tu][prow][pu];
        }
        const f32x4 c_g4 = sin4[PARV * 2 * SLOTS + slot_c];
        const float2 dh2 = sin2[PARV * 2 * SLOTS + slot_c];
        const float c_dout = dh2.x, c_hprev = dh2.y;
        const float gr = c_g4[0], gz = c_g4[1], gn = c_g4[2], ghn = c_g4[3];
        // the WORKGROUP's scale (both unit tiles: the consumers' 32-deep MFMAs span them) from the per-cell bound of gru_persist_bwd3p_kernel:
        // a wave maximum (DPP), then the eight waves' words through two tagged 16-byte LDS records
        const float carry0 = has_next ? fmaf(dh_carry, z_next, mm) : dh_carry;
        const float bnd = pok ? m3t_fin_abs((c_dout + carry0) * fmaxf(1.f, 0.25f * fabsf(ghn))) : 0.f;
        unsigned mxb = wave_umax_dpp(__float_as_uint(bnd));
        const unsigned want = (unsigned)(step + 1) & 3u;
        if (lane == 0) __hip_atomic_store(&pmx8[wave], (mxb & ~3u) | want, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const GateBwd c = gru_cell_bwd(c_dout, dh_carry, z_next, mm, has_next, gr, gz, gn, ghn, step < T - 1 ? c_hprev : 0.f);
        const float p0 = pok ? c.dr : 0.f, p1 = pok ? c.dz : 0.f, p2 = pok ? c.dnr : 0.f;
        {
            int w = 0;
            for (;;) {
                u32x4 qa, qb;
                asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)" : "=&v"(qa), "=&v"(qb) : "v"(pmx8_addr) : "memory");
                const bool all8 = ((qa.x & 3u) == want) && ((qa.y & 3u) == want) && ((qa.z & 3u) == want) && ((qa.w & 3u) == want) &&
                                  ((qb.x & 3u) == want) && ((qb.y & 3u) == want) && ((qb.z & 3u) == want) && ((qb.w & 3u) == want);
                if (all8 || dead) {
                    mxb = max(max(max(qa.x, qa.y), max(qa.z, qa.w)), max(max(qb.x, qb.y), max(qb.z, qb.w)));
                    break;
                }
                if (++w > ex.spin_limit) { dead = true; if (lane == 0) raise_spin(err, step); break; }
            }
        }
        float psc, pisc;
        m3t_f16_scale(mxb, psc, pisc);
        if (M3T_SCAN_PUBLISHES(step, RB == ROWS || plive)) {      // (rows past an 8-clip block publish nothing)
            u32x4 gq;
            gq.x = bwd3p_split(p0 * psc); gq.y = bwd3p_split(p1 * psc); gq.z = bwd3p_split(p2 * psc);
            gq.w = ((ex.tag_base + (unsigned)step + 1u) & 0xffffffu) | ((__float_as_uint(psc) >> 23) << 24);
            M3T_PUBLISH16(gran + (size_t)PARV * slot + pub, gq);
        }
        M3T_QSTAMP(4);
        dh_carry = c.dht; z_next = gz;
        sb_r += c.dr; sb_z += c.dz; sb_n += c.dn; sb_nr += c.dnr;
        if (step == amk_step) {                        // a chunk of the progress marks ends in front of this step: its magnitude slot (+ the scan's)
            if (d.amax) {
                const float m_ = wave_max(pok ? amx : 0.f);
                if (lane == 0) {
                    atomicMax(d.amax + 1 + amk, (unsigned long long)__float_as_uint(m_));
                    atomicMax(d.amax, (unsigned long long)__float_as_uint(m_));
                }
            }
            amx = 0.f;
            ++amk;
            amk_step = M3T_MARK_AT(amk);
        }
        amx = fmaxf(fmaxf(amx, m3t_fin_abs(c.dr)), fmaxf(m3t_fin_abs(c.dz), m3t_fin_abs(c.dn)));      // (|dn r| <= |dn|: one bound for dgx and dgh)
        // results to LDS; the memory-order thread stores the PREVIOUS step's (written before this step's barrier) -- after the
        // publish: the publish must not queue behind the stores
        sout[PARV * 2 * SLOTS + slot_c] = (f32x4){pok ? c.dr : 0.f, pok ? c.dz : 0.f, pok ? c.dn : 0.f, pok ? c.dnr : 0.f};
        if (step > 0 && hok) {
            const f32x4 r4 = sout[(1 - PARV) * 2 * SLOTS + slot_h];
            st_dr = r4[0]; st_dz = r4[1]; st_dn = r4[2]; st_dnr = r4[3];
            store_results(step - 1);
        }
    }
    M3T_QSTAMP(5);
}
