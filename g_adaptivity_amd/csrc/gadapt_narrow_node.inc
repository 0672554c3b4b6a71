// gadapt_narrow_node.inc - the narrow route's forward arithmetic for ONE NODE PER LANE, as a block of statements: the one definition
// that wide::fwd_narrow_kernel and wide::fwd_narrow_block_kernel (gadapt_narrow_fwd.inc) both include inside their node loops.  It is
// text and not a function on purpose: as a __forceinline__ function the same statements compile to a different instruction stream in
// fwd_narrow_kernel (about 140 more register moves and 13 more waits per instantiation), and that kernel is the route the block
// launch is measured against.
//
// In scope at the point of inclusion, every lane of the wave active:
//   t1.own, t1.rp0, t1.rp1   this lane's input row and CSR row bounds (NarrowIn)
//   xv[k], k < p.kmax        its neighbour rows (unused ELL entries: the own row)
//   af, pv[0..3]             the A fragment and p0[0..3];  h = lane / 32;  i, N: the node and the node count;  sc, dt;  p (FwdArgs)
// GADAPT_NARROW_NODE_SETTLE(Pa, Pb), optional: statements between the last MFMA and the lane swaps that read its result.  swap32 is an
// asm statement, so the compiler does not count the wait states an MFMA result needs before a VALU instruction may read it.  In
// fwd_narrow_kernel the accumulators are AGPRs and reach the swaps through v_accvgpr_read, which the compiler does guard; a kernel
// whose accumulators are VGPRs must wait here itself (fwd_narrow_block_kernel: group b's P came out wrong in the last bits without it).
// Defines: own, xc (the input row), deg, lo | hi (the new row), w[0..7] (alpha).  Each half-wave is one aligned 32-node group: its own
// MFMA group and its own half of the re-base ballot.
        // ---- P[0..3] = (A x + p0)[0..3] on the matrix cores, two 32-node groups
        const float4 own = t1.own;
        float xa[4] = {own.x, own.y, own.z, own.w}, xb[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < 4; ++c) swap32(xa[c], xb[c]);      // xa: own row in lanes 0..31, zeros above; xb: rows of lanes 32..63, moved down
        const float va[8] = {xa[0], xa[1], xa[2], xa[3], 0.f, 0.f, 0.f, 0.f};
        const float vb[8] = {xb[0], xb[1], xb[2], xb[3], 0.f, 0.f, 0.f, 0.f};
        const Split3 ba = split8(va), bb = split8(vb);
        f32x16 Pa, Pb;
#pragma unroll
        for (int q = 0; q < 16; ++q) { Pa[q] = (q < 4 && h == 0) ? pv[q & 3] : 0.f; Pb[q] = Pa[q]; }
        mfma6r(Pa, af, ba);
        mfma6r(Pb, af, bb);
#ifdef GADAPT_NARROW_NODE_SETTLE
        GADAPT_NARROW_NODE_SETTLE(Pa, Pb);                       // (see below: an includer whose MFMA results stay in VGPRs)
#endif
        float P4[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { float a = Pa[r], b = Pb[r]; swap32(a, b); P4[r] = a; }

        // ---- edge walk (wide::fwd_kernel's expressions on chunk 0)
        const int kmax = opaque(p.kmax);
        const int deg = (i < N) ? t1.rp1 - t1.rp0 : 0;
        v2f acc[2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}};
        float w[8];
        float mref = 0.f, den = 0.f;
        const v2f plo = {P4[0], P4[1]}, phi = {P4[2], P4[3]};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            w[k] = 0.f;
            if (k < kmax) {
                v2f d[4] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}, v2f{0.f, 0.f}, v2f{0.f, 0.f}};
                d[0] += plo * xv[k].xy;
                d[1] += phi * xv[k].zw;
                const v2f dd = (d[0] + d[1]) + (d[2] + d[3]);
                const float sk = ((dd.x + dd.y) + 0.f) * sc;     // (+ the wide kernel's other half: an exact +0)
                const bool valid = k < deg;
                float wk;
                if (k == 0) {
                    mref = valid ? sk : 0.f;
                    wk = valid ? 1.f : 0.f;
                } else {
                    float dlt = sk - mref;
                    const unsigned long long bal = __builtin_amdgcn_ballot_w64(valid && dlt > REBASE);
                    if ((h ? (unsigned)(bal >> 32) : (unsigned)bal) != 0u) {   // rare: re-base every node of the 32-node group
                        const float nref = valid ? fmaxf(mref, sk) : mref;
                        const float corr = sm_exp(mref - nref);
                        den *= corr;
                        acc[0] *= corr; acc[1] *= corr;
#pragma unroll
                        for (int kk = 0; kk < k; ++kk) w[kk] *= corr;
                        mref = nref;
                        dlt = sk - mref;
                    }
                    wk = valid ? sm_exp(dlt) : 0.f;
                }
                w[k] = wk;
                den += wk;
                acc[0] += xv[k].xy * wk;
                acc[1] += xv[k].zw * wk;
            }
        }
        // ---- x' = x + dt (m - x), alpha = w / (sum + 1e-16)
        const float inv = sm_rcp(den + 1e-16f);
        const v4f xc = v4f{own.x, own.y, own.z, own.w};
        v2f lo = acc[0] * inv - xc.xy, hi = acc[1] * inv - xc.zw;
        if (!p.residual_only) { lo = xc.xy + lo * dt; hi = xc.zw + hi * dt; }
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] *= inv;
