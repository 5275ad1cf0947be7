// The spectral row epilogue, in two halves (bounds the registers in flight next to the prefetched line): u_prev, v_prev and the x-pass
// partials in, residuals out.  Text of spec_ypass_kernel and spec_rowmarch_kernel: its explicit rounding sequence is what makes the fused
// and the plain row pass agree bit for bit, so it exists once; as a function template (arrays by reference) it compiles to another schedule
// in all twenty row kernels, as included text to the same instructions (DESIGN_HISTORY.md).
// In scope: NT (non-temporal streams), SEGP, TPF, pk, pbyte, base, valid, k, up, vp, ru, rv, rd, uf, vf, a, b.  Defines tu, tv.
        float tu[16], tv[16];                                            // (u - u_prev)/dt, (v - v_prev)/dt: shared by both back-ends
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float pu[8], pv[8], pd[8], qu[8], qv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const size_t ce = base + TPF * (8 * h + i);
                if constexpr (SEGP) {
                    const int so = seg_col(pk, TPF * (8 * h + i));
                    pu[i] = ld_seg<NT>(seg_rsrc(pk.pu), pbyte, so); pv[i] = ld_seg<NT>(seg_rsrc(pk.pv), pbyte, so); pd[i] = ld_seg<NT>(seg_rsrc(pk.pd), pbyte, so);
                } else {
                pu[i] = ld_stream<NT>(ru + ce); pv[i] = ld_stream<NT>(rv + ce); pd[i] = ld_stream<NT>(rd + ce);
                }
                qu[i] = ld_stream<NT>(up + ce); qv[i] = ld_stream<NT>(vp + ce);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int m = 8 * h + i;
                // explicitly rounded products: the fused and the plain instantiation must not differ by an FMA contraction here
                tu[m] = __fmul_rn(uf[m] - qu[i], k.inv_dt); tv[m] = __fmul_rn(vf[m] - qv[i], k.inv_dt);
            }
            if (valid) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const int m = 8 * h + i;
                    const size_t ce = base + TPF * m;
                    // one fixed rounding sequence (the compiler may not re-associate or contract differently per instantiation)
                    st_stream<NT>(ru + ce, __fadd_rn(__fmaf_rn(vf[m], a[m].x, __fadd_rn(tu[m], pu[i])), b[m].x));
                    st_stream<NT>(rv + ce, __fadd_rn(__fmaf_rn(vf[m], a[m].y, __fadd_rn(tv[m], pv[i])), b[m].y));
                    st_stream<NT>(rd + ce, pd[i] + a[m].y);
                }
            }
        }
