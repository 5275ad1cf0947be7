// The body of a column kernel's `field` lambda after its pin of te: field F of the spectrum y inverse-transformed along x and written to G through
// the LDS transpose.  Text of ps_col_kernel (through pspec_col_pass.inc; F = 4, 5: the scalar's gradient), ps_col_adj_kernel (F = 4, 5: kappa's;
// with a PsAdjScalar F = 6, 7: the state's scalar; 8, 9: its cotangent m).
// F is the field of G that is written, FK which spectrum it is (0: u^, 1: v^, from 2 on the gradient's x and y part by parity): FK = F but in
// the tangent's pass of ps_col_kernel, whose velocity and gradient are G fields 4-7 (FK = F - 4; U0 = V0 = 0 there).
// In scope: the names of pspec_col_tile.inc, F, FK, y, te, tv, ky, U0, V0, a, tab, G, my1, TPF, RPI.
                cf o[16];
#pragma unroll
                for (int m = 0; m < 16; ++m) {
                    const int e = te + TPF * m;
                    const int mx = m < 8 ? e : e - N;
                    const float kx = a.kx1 * (float)mx;
                    const float k2 = kx * kx + ky * ky;
                    const float ik2 = k2 > 0.f ? a.inv_n / k2 : 0.f;
                    if constexpr (FK == 0) o[m] = imul(ky * ik2, y[m]);                // u^ = i ky psi^
                    else if constexpr (FK == 1) o[m] = imul(-kx * ik2, y[m]);          // v^ = -i kx psi^
                    else if constexpr (FK % 2 == 0) o[m] = imul(kx * a.inv_n, y[m]);    // (w_x)^, (theta_x)^: the even fields from 2 on
                    else o[m] = imul(ky * a.inv_n, y[m]);                              // (w_y)^, (theta_y)^: the odd ones
                }
                if constexpr (FK < 2) {
                    if (te == 0 && lj == 0) o[0] = {F == 0 ? U0 : V0, 0.f};           // the mean flow in the (0, 0) mode
                }
                fft_line<float, N, true>(o, tab, tab + N / 2, xb, tv);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
#pragma unroll
                for (int m = 0; m < 16; ++m) { mine[2 * (tv + TPF * m)] = o[m].x; mine[2 * (tv + TPF * m) + 1] = o[m].y; }
                __syncthreads();
                if (sok) {
                    float2* g = G + (size_t)F * a.fstride + sbase;
                    for (int r = cr; r < N; r += RPI) g[(size_t)r * my1] = make_float2(cp[2 * r], cp[2 * r + 1]);
                }
                __syncthreads();
