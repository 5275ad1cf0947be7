// Tile t of a column-pass launch -> lt, its place in the walk, and j0, its first column (the four column kernels; each adds its own grid offset g,
// whose form differs: segmented or not).  Neighbouring tiles run on the same XCD (they share 128-byte lines), and the tiles are walked from the
// LAST grid to the first (see launch_xpass, spectral_fwd.h).  In scope: t, ntiles, tiles_per_grid, CW (columns per tile), j0 (declared).
// (As a function of scalars the grid stride is evaluated before the walk, and every column kernel compiles to another schedule.)
        const long lt = ntiles - 1 - (long)xcd_remap((unsigned)t, (unsigned)ntiles);
        j0 = (int)(lt % tiles_per_grid) * CW;
