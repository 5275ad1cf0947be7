// A transform wave's place in a column tile, recomputed per tile from an opaque copy of the thread id (cheaper than the spill / reload the compiler
// otherwise chooses for values live across the whole tile body).  Text of the four column kernels (spec_xpass_kernel, spec_xpass_split_kernel,
// spec_bwd_xpass_kernel, spec_bwd_xsplit_kernel).  In scope: L, TPF, lines, CL (the kernel's LDS layout: SpecLds or SplitLds).
// Defines tx, wave, lane, sub, tid, line, xb (the line's exchange image) and my_stage (its skewed, conflict-free staging image, [field][row]).
        int tx = threadIdx.x;
        asm volatile("" : "+v"(tx));
        const int wave = tx / kWave, lane = tx % kWave;
        const int sub = lane / TPF, tid = lane % TPF;
        const int line = wave * L::FPW + sub;
        unsigned char* xb = lines + (size_t)line * CL::LINE_BYTES;
        float* my_stage = reinterpret_cast<float*>(xb) + (line % CL::SKEW_MOD) * CL::SKEW_DW;
