// One point of the FD 5-point residual in the fused row passes (fd_residual's formula).  Text of spec_ypass_kernel<.., FUSE_FD> and
// spec_rowmarch_kernel: as a function of scalars it compiles to other registers in the marching kernel (DESIGN_HISTORY.md).
// In scope: m (the slot), tu, tv (kept from the spectral epilogue), fk, fu, fv, fd, co (the point's element offset) and the stencil's values:
// ucc, vcc (centre), ul, vl, p_l / ur, vr, p_r (columns j-1 / j+1), u_m, v_m, p_m / u_n, v_n, p_n (rows i-1 / i+1).  The sites compute the
// column neighbours themselves (lane rotates): where they stand in the text decides the marching kernel's registers.
                        const float ux = (u_n - u_m) * fk.inv_2dx, uy = (ur - ul) * fk.inv_2dy;
                        const float vx = (v_n - v_m) * fk.inv_2dx, vy = (vr - vl) * fk.inv_2dy;
                        const float px = (p_n - p_m) * fk.inv_2dx, py = (p_r - p_l) * fk.inv_2dy;
                        // second differences as (a - c) - (c - b): neighbouring values of a resolved field are within a factor 2 of each
                        // other, so both first differences are EXACT in float32 (Sterbenz) and the only rounding is relative to the second
                        // difference itself -- the accuracy of the float64 sum without ~28 double-rate instructions per point
                        // (these passes are VALU-issue-bound, unlike the standalone stencil kernel, which keeps the float64 form)
                        const float lu = ((u_n - ucc) - (ucc - u_m)) * fk.inv_dx2f + ((ur - ucc) - (ucc - ul)) * fk.inv_dy2f;
                        const float lv = ((v_n - vcc) - (vcc - v_m)) * fk.inv_dx2f + ((vr - vcc) - (vcc - vl)) * fk.inv_dy2f;
                        st_stream<true>(fu + co, tu[m] + ucc * ux + vcc * uy + px * fk.inv_rho - fk.nu * lu);
                        st_stream<true>(fv + co, tv[m] + ucc * vx + vcc * vy + py * fk.inv_rho - fk.nu * lv);
                        st_stream<true>(fd + co, ux + vy);
