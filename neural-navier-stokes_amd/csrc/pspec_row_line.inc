// One line of a row kernel, as text of ps_row_kernel and ps_row_adj_kernel (a type that holds these compiles to other code there): lane tid of
// the TPF that share grid row `row` (clamped; valid: the row exists), its exchange image xb and the row's G field 0, g0.
// In scope: L (PsLds<N>), TPF, lines, it, a, G, my1.
        int tx = threadIdx.x;
        asm volatile("" : "+v"(tx));
        const int wave = tx / kWave, lane = tx % kWave, sub = lane / TPF, tid = lane % TPF;
        const int line = wave * L::FPW + sub;
        cf* xb = reinterpret_cast<cf*>(lines + (size_t)line * L::LINE_BYTES);
        const long row_raw = it * L::LINES + line;
        const bool valid = row_raw < a.nlines;
        const long row = valid ? row_raw : a.nlines - 1;
        const float2* g0 = G + (size_t)row * my1;
