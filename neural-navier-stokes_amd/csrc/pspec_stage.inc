// The staged forward transform of a column tile: Ph's field ph through the LDS transpose into z[16], then forward-transformed along x.  Text of
// ps_col_kernel (through pspec_col_pass.inc), ps_col_adj_kernel and ps_transfer_kernel: as a function or a lambda it compiles to other registers
// in ps_col_kernel.  In scope: the names of pspec_col_tile.inc, ph, z, my1, tab, tv, TPF, RPI.
            for (int r = cr; r < N; r += RPI) {
                const float2 v = sok ? ph[sbase + (size_t)r * my1] : make_float2(0.f, 0.f);
                cp[2 * r] = v.x; cp[2 * r + 1] = v.y;
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < 16; ++m) z[m] = {mine[2 * (tv + TPF * m)], mine[2 * (tv + TPF * m) + 1]};
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            fft_line<float, N, false>(z, tab, tab + N / 2, xb, tv);
