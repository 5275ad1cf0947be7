// Memory waves: the first tile's three input fields, registers R[0 .. 2] -> the staging image (spectral_split_mem.inc), then the barrier the
// transform waves wait at.  In scope: R, NR, MROWS, SF, stage.
#pragma unroll
        for (int q = 0; q < NR / 4; ++q)
#pragma unroll
            for (int f = 0; f < 3; ++f)
                *reinterpret_cast<float4*>(stage + f * SF + 4 * MROWS * q) = make_float4(R[f][4 * q], R[f][4 * q + 1], R[f][4 * q + 2], R[f][4 * q + 3]);
        __syncthreads();                                                        // inputs of the first tile are staged
