// A memory wave's place in the role-split column kernels (spec_xpass_split_kernel, spec_bwd_xsplit_kernel).  A memory lane owns rows
// 4 cr .. 4 cr + 3 of every block of 4 MROWS rows: element i <-> row 4 cr + (i & 3) + 4 MROWS (i >> 2), so that its four consecutive rows move
// through LDS as ONE 16-byte access (24 + 24 LDS instructions per exchange instead of 96 + 96).
// In scope: CW, SL, lines.  Defines mt, cc, cr, stage (this lane's column of the staging image, [field][row]).
        int mt = threadIdx.x - kSpecThreads;
        asm volatile("" : "+v"(mt));
        const int cc = mt % CW, cr = mt / CW;
        float* stage = reinterpret_cast<float*>(lines + (size_t)cc * SL::LINE_BYTES) + (cc % 8) * SL::SKEW_DW + 4 * cr;       // [field][row]
