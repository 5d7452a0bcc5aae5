// One step of gru_persist_bwd16_kernel, the backward scan of the bf16 mode (included twice: even steps read the activation set A and request B, odd steps
// the reverse).  STEPV = the step index, CUR(x) / NXT(x) = the register set in use / being filled.
{
    const int step = STEPV;
    const bool has_next = step > 0;
    M3T_STAMP(0);
    if (has_next) {
        const unsigned tag = (ex.tag_base + (unsigned)step) & 0xffffu;
        const unsigned long long* src = gran + (size_t)((step - 1) & 1) * slot + grp + lane_off;
        pu32x4 v[KS][4];                               // [k-step][unit pair jp] = {lo(j0), hi(j0), lo(j1), hi(j1)}
        int spins = 0;
        M3T_GATHER_DELAY(step);
        for (;;) {
#pragma unroll
            for (int k = 0; k < KS; ++k) {
                const unsigned long long* qp = src + (size_t)(2 * k) * NW * TILE;
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
                for (int jp = 0; jp < 4; ++jp) {
                    asm volatile("" : "+v"(v[k][jp]));
                    ok = ok && ((v[k][jp].y >> 16) == tag) && ((v[k][jp].w >> 16) == tag);
                }
            M3T_GATHER_RETRY(ok, step);
        }
        gather_note_fail(spins, lane, &poll_fail[step & 1]);
        // this step's activations (requested one step ago) are complete since the vmcnt(0) above
        asm volatile("" : "+v"(CUR(dout)), "+v"(CUR(g4)), "+v"(CUR(hprev)));
        M3T_STAMP(1);
        f32x4 acc = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KS; ++k) {
            pu32x4 ar, az, an;                             // dr, dz, dn*r of 8 consecutive units, paired into dwords
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                ar[jj] = __builtin_amdgcn_perm(v[k][jj].z, v[k][jj].x, 0x05040100u);
                az[jj] = __builtin_amdgcn_perm(v[k][jj].z, v[k][jj].x, 0x07060302u);
                an[jj] = __builtin_amdgcn_perm(v[k][jj].w, v[k][jj].y, 0x05040100u);
            }
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pbf16x8, ar), wb[k][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pbf16x8, az), wb[k][1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(pbf16x8, an), wb[k][2], acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) red[step & 1][wave][(lane >> 4) * 4 + r][lane & 15] = acc[r];
    }
    cell_phase_wait();
    // every step, unconditionally (a conditional definition gets merged by copies that read registers in flight): with
    // nothing else outstanding, request the next step's activations -- a whole step to arrive
    M3T_BWD_LOAD_STEP(step + 1, NXT(dout), NXT(g4), NXT(hprev));
    M3T_STAMP(2);
    __syncthreads();
    M3T_POLL_ADAPT(step & 1, (step + 1) & 1, step);
    M3T_STAMP(3);
    if (pw) {
        float mm = 0.f;
        if (has_next) {
#pragma unroll
            for (int w = 0; w < NW; ++w) mm += red[step & 1][w][prow][pu];
        }
        const float gr = CUR(g4).x, gz = CUR(g4).y, gn = CUR(g4).z, ghn = CUR(g4).w;
        const GateBwd c = gru_cell_bwd(CUR(dout), dh_carry, z_next, mm, has_next, gr, gz, gn, ghn, step < T - 1 ? CUR(hprev) : 0.f);
        if (M3T_SCAN_PUBLISHES(step, true)) {             // 8-byte granule {bf16 dr, bf16 dz, bf16 dn*r, tag16}: the values ARE bf16 in this mode
            const unsigned lo = (__float_as_uint(pok ? rbf(c.dr) : 0.f) >> 16) | (__float_as_uint(pok ? rbf(c.dz) : 0.f) & 0xffff0000u);
            const unsigned hi = (__float_as_uint(pok ? rbf(c.dnr) : 0.f) >> 16) | (((ex.tag_base + (unsigned)step + 1u) & 0xffffu) << 16);
            const unsigned long long gq = ((unsigned long long)hi << 32) | lo;
            M3T_PUBLISH8(gran + (size_t)(step & 1) * slot + pub, gq);
        }
        M3T_MARK_PUBLISHED(step);
        M3T_STAMP(4);
        dh_carry = c.dht; z_next = gz;
        sb_r += c.dr; sb_z += c.dz; sb_n += c.dn; sb_nr += c.dnr;
        st_dr = c.dr; st_dz = c.dz; st_dn = c.dn; st_dnr = c.dnr;
        if (pok) store_results(step);              // after the publish: the publish must not queue behind them
    }
    M3T_STAMP(5);
}
