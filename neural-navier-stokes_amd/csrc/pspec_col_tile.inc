// A thread's two roles in column tile t of CW columns, as text of ps_col_kernel, ps_col_adj_kernel and ps_transfer_kernel (a type that holds
// these compiles to other code there).  Transform role: lane tid of the TPF that share line `line`, which is column lcol = (lb, lj) (lok: it
// exists) at wbase in the layout of W, with its exchange image xb and its skewed staged image `mine`.
// In scope: L (PsLds<N>), TPF, CW, lines, tx (the thread), t, a, my1.
        const int wave = tx / kWave, lane = tx % kWave, sub = lane / TPF, tid = lane % TPF;
        const int line = wave * L::FPW + sub;
        cf* xb = reinterpret_cast<cf*>(lines + (size_t)line * L::LINE_BYTES);
        float* mine = reinterpret_cast<float*>(xb) + (line % L::SKEW_MOD) * L::SKEW_DW;
        // staging role: thread (cc, cr) moves rows cr, cr + RPI, ... of tile column cc
        const int cc = tx % CW, cr = tx / CW;
        float* cp = reinterpret_cast<float*>(lines + (size_t)cc * L::LINE_BYTES) + (cc % L::SKEW_MOD) * L::SKEW_DW;
        const long scol = t * CW + cc;
        const bool sok = scol < a.nlines;
        const size_t sbase = sok ? (size_t)(scol / my1) * N * my1 + (size_t)(scol % my1) : 0;     // (b, i = 0, j) in [b][i][j]
        // transform role: this line is column lcol = (b, j)
        const long lcol = t * CW + line;
        const bool lok = lcol < a.nlines;
        [[maybe_unused]] const int lb = lok ? (int)(lcol / my1) : 0, lj = lok ? (int)(lcol % my1) : 0;
        const size_t wbase = (size_t)(lok ? lcol : 0) * N;
