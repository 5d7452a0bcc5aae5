// One step of gru_persist_bwd_kernel (included twice: even steps read the activation set A and request B, odd steps
// the reverse).  STEPV = the step index, CUR(x) / NXT(x) = the register set in use / being filled.
{
    const int step = STEPV;
    const bool has_next = step > 0;
    M3T_STAMP(0);
    if (has_next) {
        const unsigned tag = ex.tag_base + (unsigned)step;
        const u32x4* src = gran + (size_t)((step - 1) & 1) * slot + grp + (size_t)wave * TILE + lane;
        u32x4 v[NC][RT][4];
        int spins = 0;
        M3T_GATHER_DELAY(step);
        for (;;) {
#pragma unroll
            for (int m = 0; m < NC; ++m)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const u32x4* q = src + (size_t)m * NW * TILE + rt * 256;
                    asm volatile("global_load_dwordx4 %0, %4, off sc1\n\t"
                                 "global_load_dwordx4 %1, %4, off offset:1024 sc1\n\t"
                                 "global_load_dwordx4 %2, %4, off offset:2048 sc1\n\t"
                                 "global_load_dwordx4 %3, %4, off offset:3072 sc1"
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
                        ok = ok && (v[m][rt][e].w == tag);
                    }
            M3T_GATHER_RETRY(ok, step);
        }
        gather_note_fail(spins, lane, &poll_fail[step & 1]);
        // this step's activations (requested one step ago) are complete since the vmcnt(0) above
        asm volatile("" : "+v"(CUR(dout)), "+v"(CUR(g4)), "+v"(CUR(hprev)));
        M3T_STAMP(1);
        f32x4 acc[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) acc[rt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int gt = 0; gt < 3; ++gt)             // ascending chunk order gate*nchh + wave + 8m: as the per-step kernel
#pragma unroll
            for (int m = 0; m < NC; ++m)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(v[m][rt][0][gt]), wt[gt][m].x, acc[rt], 0, 0, 0);
                    acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(v[m][rt][1][gt]), wt[gt][m].y, acc[rt], 0, 0, 0);
                    acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(v[m][rt][2][gt]), wt[gt][m].z, acc[rt], 0, 0, 0);
                    acc[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(v[m][rt][3][gt]), wt[gt][m].w, acc[rt], 0, 0, 0);
                }
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[step & 1][wave][rt * 16 + (lane >> 4) * 4 + r][lane & 15] = acc[rt][r];
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
        if (M3T_SCAN_PUBLISHES(step, true)) {             // 16-byte granule {dr, dz, dn*r, tag32}
            u32x4 gq;
            const bool bf = g.bf16 != 0;
            gq.x = __float_as_uint(pok ? (bf ? rbf(c.dr) : c.dr) : 0.f); gq.y = __float_as_uint(pok ? (bf ? rbf(c.dz) : c.dz) : 0.f);
            gq.z = __float_as_uint(pok ? (bf ? rbf(c.dnr) : c.dnr) : 0.f); gq.w = ex.tag_base + (unsigned)step + 1u;
            M3T_PUBLISH16(gran + (size_t)(step & 1) * slot + pub, gq);
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
