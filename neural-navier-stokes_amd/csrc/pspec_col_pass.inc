// One field's pass through a column tile of ps_col_kernel (pspec_kernels.hip), which includes this text once per field with TH in scope:
// TH = false the vorticity (Ph field 0, W / A, G fields 0..3), TH = true the scalar (Ph field 1, theta^ / A_theta, G fields 4 and 5), TG = true
// (TH = false) the tangent (Ph field 1, dw^ / dA with the vorticity's factors and mask, dg^ where the vorticity adds g^, no kick, no mean
// flow, its four spectra to G fields 4..7).  TANSC (a PsScalar and a PsTangentScalar in the pack: the tangent of the scalar system) has four
// fields: the vorticity, the scalar, then TG alone on Ph field 2 and G fields 6..9 and TH with TG, the scalar's perturbation: Ph field 3,
// dtheta^ / dA_theta with E_theta and the mask that keeps (0, 0), no g^, no dg^, no kick, zero means, its gradient to G fields 10 and 11.  TANSCS
// (K pairs on one base) includes those two passes in a loop's scope where TANSC is true and Ph, G, tg, dTh, dAt are member k's.  Plain
// text rather than a function or a lambda: the unscalared kernels then compile to the instructions they had before there was a scalar
// (a lambda's body is optimised on its own before it is inlined, and came out a few instructions and registers different).
// STOCH (ps_col_kernel's note) is false in every kernel without a PsStoch argument, whose text below is then what it was.
// LINEAR likewise (a PsLinear argument): the vorticity's factors E - 1, E^2 - 1 are then complex, from the table lin, and scal's complex form applies.
// STAGES likewise (a PsKeep, a PsKeepScalar or a PsKeepTangent argument): stages 1-3 also store the next stage's input to stage_out (the scalar's
// to tstage_out, the tangent's to dstage_out).
// The staged forward transform and the field emit are text of their own (pspec_stage.inc, pspec_field.inc), shared with ps_col_adj_kernel and
// ps_transfer_kernel; the tile's names (lok, lj, wbase, sok, ...) are those of pspec_col_tile.inc.
{
        constexpr int PF = TANSC ? (TG ? 2 : 0) + (TH ? 1 : 0) : TH || TG ? 1 : 0;     // the field of Ph this pass consumes
        const float2* ph = PF == 0 ? Ph : PF == 1 ? Ph + a.fstride : Ph + PF * a.fstride;
        float2* Ws = TG ? (TH ? dTh : tg.dW) : TH ? Th : W;
        float2* As = TG ? (TH ? dAt : tg.dA) : TH ? At : A;
        cf y[16];
        if constexpr (S == 0) {
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const float2 w = lok ? Ws[wbase + tv + TPF * m] : make_float2(0.f, 0.f);
                y[m] = {w.x, w.y};
            }
        } else {
            cf z[16];
#include "pspec_stage.inc"
            int te = tv;
            asm volatile("" : "+v"(te), "+v"(z[0].x));
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const int e = te + TPF * m;
                const int mx = m < 8 ? e : e - N;
                // 2/3 rule in x (y: j < my1); the vorticity has no (0, 0) mode, the scalar keeps it (its mean)
                const bool keep = lok && 3 * (mx < 0 ? -mx : mx) < N && (TH || (mx | lj) != 0);
                [[maybe_unused]] const float kx = a.kx1 * (float)mx;
                std::conditional_t<LINEAR && !TH, cf, float> em1, em2;             // E - 1, E^2 - 1
                if constexpr (LINEAR && !TH) {
                    const float2 l = keep ? lin[(size_t)lj * N + e] : make_float2(0.f, 0.f);   // lambda dt / 2: lane-owned, coalesced, like g^
                    ps_linear_factors(l, em1, em2);
                } else {
                    float x = (TH ? hkdt : a.hnudt) * (kx * kx + ky * ky);         // L dt / 2
                    if constexpr (FORCED && !TH) x -= fc.hdrag;
                    em1 = expm1f(x); em2 = expm1f(2.f * x);
                }
                cf n = keep ? cf{-z[m].x, -z[m].y} : cf{0.f, 0.f};
                if constexpr (TH && TG) {               // dN_theta has no (0, 0) mode (div u = 0, du has no mean to meet G): exactly, not to rounding,
                    if ((mx | lj) == 0) n = {0.f, 0.f}; // so the mean of dtheta is carried bit for bit
                }
                if constexpr (FORCED && !TH && !TG) {
                    const float2 g = gok ? fc.g[gbase + e] : make_float2(0.f, 0.f);
                    if (keep) n = {n.x + g.x, n.y + g.y};
                }
                if constexpr (TG && !TH) {              // the source's perturbation, where the vorticity adds g^; the unforced base has none of its own
                    const float2 g = dgok ? tg.dg[dgbase + e] : make_float2(0.f, 0.f);
                    if (keep) n = {n.x + g.x, n.y + g.y};
                }
                const size_t si = wbase + e;
                if constexpr (S == 1) {                 // a: A = E^2 (w + dt/6 a), next = E (w + dt/2 a)
                    const float2 w2 = lok ? Ws[si] : make_float2(0.f, 0.f);
                    const cf w = keep ? cf{w2.x, w2.y} : cf{0.f, 0.f};
                    const cf acc = scal(em2, axpy(dt6, n, w));
                    if (lok) As[si] = make_float2(acc.x, acc.y);
                    y[m] = scal(em1, axpy(dt2, n, w));
                } else if constexpr (S == 2) {          // b: A += dt/3 E b, next = E w + dt/2 b
                    const float2 w2 = lok ? Ws[si] : make_float2(0.f, 0.f), a2 = lok ? As[si] : make_float2(0.f, 0.f);
                    const cf w = keep ? cf{w2.x, w2.y} : cf{0.f, 0.f};
                    const cf acc = axpy(dt3, scal(em1, n), cf{a2.x, a2.y});
                    if (lok) As[si] = make_float2(acc.x, acc.y);
                    y[m] = axpy(dt2, n, scal(em1, w));
                } else if constexpr (S == 3) {          // c: A += dt/3 E c, next = E^2 w + dt E c
                    const float2 w2 = lok ? Ws[si] : make_float2(0.f, 0.f), a2 = lok ? As[si] : make_float2(0.f, 0.f);
                    const cf w = keep ? cf{w2.x, w2.y} : cf{0.f, 0.f};
                    const cf ec = scal(em1, n);
                    const cf acc = axpy(dt3, ec, cf{a2.x, a2.y});
                    if (lok) As[si] = make_float2(acc.x, acc.y);
                    y[m] = axpy(dt, ec, scal(em2, w));
                } else {                                // d: w = A + dt/6 d
                    const float2 a2 = lok ? As[si] : make_float2(0.f, 0.f);
                    const cf acc = keep ? cf{a2.x, a2.y} : cf{0.f, 0.f};
                    cf w = axpy(dt6, n, acc);
                    if constexpr (STOCH && !TH && !TG) { // the kick of the finished step: w += sqrt(dt) a xi, Philox only on the forced ring
                        const float amp = keep ? samp[(size_t)lj * N + e] : 0.f;
                        if (amp != 0.f) {
                            const bool mirror = lj == 0 && mx < 0;                 // the j = 0 line stores -m_x too: |m_x|'s sample, conjugated
                            const cf xi = ps_normal(sn0, sn1, (unsigned)(lj * N + (mirror ? -mx : e)), sid, sk0, sk1);
                            const float sa = sqdt * amp;
                            w = {fmaf(sa, xi.x, w.x), fmaf(mirror ? -sa : sa, xi.y, w.y)};
                        }
                    }
                    if (lok) Ws[si] = make_float2(w.x, w.y);
                    y[m] = w;
                }
                if constexpr (STAGES && TG) {
                    if (lok) dstage_out[si] = make_float2(y[m].x, y[m].y);
                } else if constexpr (STAGES) {
                    if (lok) (TH ? tstage_out : stage_out)[si] = make_float2(y[m].x, y[m].y);
                }
            }
        }
        if (S < 4 || emit) {
            const float U0 = !TH && !TG && lok ? mean[2 * lb] : 0.f, V0 = !TH && !TG && lok ? mean[2 * lb + 1] : 0.f;
            auto field = [&](auto fc) {
                constexpr int F = decltype(fc)::value, FK = TG && !TH ? F - (TANSC ? 6 : 4) : F;      // the tangent's four spectra go to G fields 4-7 (TANSC: 6-9)
                int te = tv;
                asm volatile("" : "+v"(te), "+v"(y[0].x));
#include "pspec_field.inc"
            };
            if constexpr (TG && TH) static_for<10, 12>(field);
            else if constexpr (TG && TANSC) static_for<6, 10>(field);
            else if constexpr (TG) static_for<4, 8>(field);
            else if constexpr (TH) static_for<4, 6>(field);
            else static_for<0, 4>(field);
        } else {
            __syncthreads();                        // the next staging overwrites line images other waves may still read
        }
}
