// The viscous filter next to spectral_filter_m1.inc (include that first: ke, ct come from it):
//     -nu k^2 FFT(f) = (br + i bi) D = -F2 D,   F2 = -(nu k / 2)(k + i k cot(theta / 2)) = -i nu k M1;   the site multiplies:
//     (br zv.x - bi zv.y,  br zv.y + bi zv.x)
// (amplification nu k relative to M1).  In scope besides: c2h (half the viscous factor per unit squared wavenumber index).
            const float kf = (float)ke * c2h;
            const float br = kf * (float)ke, bi = kf * ct;
