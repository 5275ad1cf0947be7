// One spectrum's pass through a column tile of ps_col_adj_kernel (pspec_kernels.hip; its note has the recurrences), which includes this text
// once per spectrum with TH in scope, the way ps_col_kernel includes pspec_col_pass.inc: TH = false the vorticity (Ph fields 0 and 1,
// lam / wbar / gbar, grad kappa to G fields 4 and 5), TH = true the scalar (a PsAdjScalar's; Ph field 2, mu / thetabar, grad m to G fields 8
// and 9).  The scalar's arithmetic differs in three places: L dt / 2 = hkdt |k|^2 without the drag, the mask keeps the (0, 0) mode, and
// r_theta is Ph's third field as it stands (no inverse Laplacian, no source to sum a cotangent for).
// LINEAR (ps_col_adj_kernel's note) is false in every kernel without a table, whose text below is then what it was; with one the vorticity's
// factors are conj(E) - 1, conj(E^2) - 1 from the table and scal's complex form applies.  The scalar's stay real.
// OPERATOR (a PsAdjOperator / PsAdjScalarOperator, LINEAR with it) is false in every other kernel, whose text is then what it was; with one
// the vorticity's pass of stages 3-1 also sums the table's cotangent of the step in ad.lstep and adds it to ad.lbar, lane-owned like gbar.
// TD (ps_col_adj_kernel's SECOND form, TH false with it) is false in every other kernel, whose code is then what it was; with it the pass is the
// vorticity's on the second quadruple: Ph fields 2 and 3, dlam / dwbar / dgbar (ginit starts dgbar as it starts gbar), grad dkappa to G fields
// 10 and 11.  The sum of kappa has its statements twice, for ad.gbar and for ad.dgbar: one pointer chosen at the head of the pass compiled the
// flow's stage 4 to other instructions.
// In scope: the names of pspec_col_tile.inc, consume, field, ad (PsAdj; PsAdjScalar where TH is true, PsAdjSecond where TD is), tv, ky, dt, dt2, dt3, dt6.
{
        float2* lamp;
        float2* barp;
        if constexpr (TD) {
            lamp = ad.dlam;
            barp = ad.dwbar;
        } else if constexpr (TH) {
            lamp = ad.mu;
            barp = ad.tbar;
        } else {
            lamp = ad.lam;
            barp = ad.wbar;
        }
        [[maybe_unused]] cf kap[16];
        if constexpr (S < 4) {
            cf r[16];
            [[maybe_unused]] cf z[16];
            if constexpr (TH) {
                consume(Ph + 2 * a.fstride, r);
            } else if constexpr (TD) {
                consume(Ph + 2 * a.fstride, r);
                __syncthreads();                    // the next staging overwrites line images other waves may still read
                consume(Ph + 3 * a.fstride, z);
            } else {
                consume(Ph, r);
                __syncthreads();                    // the next staging overwrites line images other waves may still read
                consume(Ph + a.fstride, z);
            }
            int te = tv;
            asm volatile("" : "+v"(te), "+v"(r[0].x));
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int e = te + TPF * m;
                const int mx = m < 8 ? e : e - N;
                const bool keep = lok && 3 * (mx < 0 ? -mx : mx) < N && (TH || (mx | lj) != 0);
                const float kx = a.kx1 * (float)mx;
                const float k2 = kx * kx + ky * ky;
                std::conditional_t<LINEAR && !TH, cf, float> em1, em2;               // E - 1, E^2 - 1; LINEAR: of conj(E), the transpose of E
                if constexpr (LINEAR && !TH) {
                    const float2 l = keep ? ad.lin[(size_t)lj * N + e] : make_float2(0.f, 0.f);   // lambda dt / 2: the forward's load
                    ps_linear_factors(l, em1, em2);
                    em1.y = -em1.y; em2.y = -em2.y;
                } else {
                    float x;                                                         // L dt / 2
                    if constexpr (TH) x = ad.hkdt * k2;
                    else x = a.hnudt * k2 - ad.hdrag;
                    em1 = expm1f(x); em2 = expm1f(2.f * x);
                }
                cf rr = {0.f, 0.f};
                if constexpr (TH) {
                    if (keep) rr = r[m];
                } else {
                    const float ik2 = k2 > 0.f ? 1.f / k2 : 0.f;
                    if (keep) rr = {fmaf(-ik2, z[m].x, r[m].x), fmaf(-ik2, z[m].y, r[m].y)};
                }
                const size_t si = wbase + e;
                const float2 l2 = lok ? lamp[si] : make_float2(0.f, 0.f);
                const cf lam = keep ? cf{l2.x, l2.y} : cf{0.f, 0.f};
                cf wb;
                if constexpr (S == 3) {
                    wb = scal(em2, cf{lam.x + rr.x, lam.y + rr.y});
                    kap[m] = scal(em1, axpy(dt, rr, cf{dt3 * lam.x, dt3 * lam.y}));
                } else {
                    const float2 w2 = lok ? barp[si] : make_float2(0.f, 0.f);
                    if constexpr (S == 0) {
                        wb = {w2.x + rr.x, w2.y + rr.y};
                    } else {
                        const cf er = scal(em1, rr);
                        wb = {w2.x + er.x, w2.y + er.y};
                        if constexpr (S == 2) {
                            const cf el = scal(em1, lam);
                            kap[m] = axpy(dt2, rr, cf{dt3 * el.x, dt3 * el.y});
                        } else {
                            const cf el = scal(em2, lam);
                            kap[m] = axpy(dt2, er, cf{dt6 * el.x, dt6 * el.y});
                        }
                    }
                }
                if constexpr (OPERATOR && !TH) {
                    // the table's cotangent (ps_col_adj_kernel's note): c conj(D) for every z = D dl this stage holds the cotangent c of; only
                    // conj(E), conj(E^2) appear (conj(E w0) = conj(E) conj(w0)); lam and rr are zero off the kept modes, and so is lbar
                    if (lok) {
                        const float2 so = ad.own[si];
                        cf add;
                        if constexpr (S == 3) {
                            const float2 w0 = ad.w0[si];
                            const cf ew = scal(em2, cf{w0.x, -w0.y});
                            add = cmul(axpy(1.f / 3.f, lam, rr), cf{so.x + ew.x, ew.y - so.y});
                        } else if constexpr (S == 2) {
                            const float2 w0 = ad.w0[si];
                            const cf ls = cmul(lam, cf{so.x, -so.y});
                            add = scal(em1, axpy(2.f / 3.f, ls, cmul(rr, cf{w0.x, -w0.y})));
                        } else {
                            add = cmul(axpy(2.f / 3.f, scal(em1, lam), rr), cf{so.x, -so.y});
                        }
                        if constexpr (S == 3) {
                            ad.lstep[si] = make_float2(add.x, add.y);
                        } else {
                            const float2 p2 = ad.lstep[si];
                            if constexpr (S == 2) {
                                ad.lstep[si] = make_float2(p2.x + add.x, p2.y + add.y);
                            } else {                       // the step's sum is complete: to the call's
                                const float2 b2 = ad.ginit ? make_float2(0.f, 0.f) : ad.lbar[si];
                                ad.lbar[si] = make_float2(b2.x + (p2.x + add.x), b2.y + (p2.y + add.y));
                            }
                        }
                    }
                }
                if (lok) {
                    if constexpr (S == 0) {
                        lamp[si] = make_float2(wb.x, wb.y);
                    } else {
                        barp[si] = make_float2(wb.x, wb.y);
                        if constexpr (TD) {
                            if (ad.dgbar) {
                                const float2 g2 = ad.dgbar[si];
                                ad.dgbar[si] = make_float2(g2.x + kap[m].x, g2.y + kap[m].y);
                            }
                        } else if constexpr (!TH) {
                            if (ad.gbar) {
                                const float2 g2 = ad.gbar[si];
                                ad.gbar[si] = make_float2(g2.x + kap[m].x, g2.y + kap[m].y);
                            }
                        }
                    }
                }
            }
        } else {
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int e = tv + TPF * m;
                const int mx = m < 8 ? e : e - N;
                const bool keep = lok && 3 * (mx < 0 ? -mx : mx) < N && (TH || (mx | lj) != 0);
                const size_t si = wbase + e;
                const float2 l2 = lok ? lamp[si] : make_float2(0.f, 0.f);
                kap[m] = keep ? cf{dt6 * l2.x, dt6 * l2.y} : cf{0.f, 0.f};
                if constexpr (TD) {
                    if (lok && ad.dgbar) {
                        const float2 g2 = ad.ginit ? make_float2(0.f, 0.f) : ad.dgbar[si];
                        ad.dgbar[si] = make_float2(g2.x + kap[m].x, g2.y + kap[m].y);
                    }
                } else if constexpr (!TH) {
                    if (lok && ad.gbar) {
                        const float2 g2 = ad.ginit ? make_float2(0.f, 0.f) : ad.gbar[si];
                        ad.gbar[si] = make_float2(g2.x + kap[m].x, g2.y + kap[m].y);
                    }
                }
            }
        }
        if constexpr (S >= 1) {
            static_for<TD ? 10 : TH ? 8 : 4, TD ? 12 : TH ? 10 : 6>([&](auto fc) { field(fc, kap); });
        } else {
            __syncthreads();                        // the next staging overwrites line images other waves may still read
        }
}
