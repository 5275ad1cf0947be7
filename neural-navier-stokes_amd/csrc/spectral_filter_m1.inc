// Slot m of the all-float32 mode's first-derivative filter on a forward-DIFFERENCED transform zv = FFT(d) (diff_fft):
//     i k FFT(f) = M1 D,   M1 = (k / 2)(cot(theta / 2) - i) = ar - i ai:   BOUNDED, no noise amplification.  The site multiplies:
//     (ar zv.x + ai zv.y,  ar zv.y - ai zv.x),  in its own statement order (x multiplied and stored, then y: the order decides the schedule).
// Text of deriv_core (velocity), adj_core and spec_bwd_xsplit_kernel, inside their static_for over the slots: as functions of (te, ctab, c1h,
// zv[m]) that return the product, the filters compile to another schedule in every float32 kernel (DESIGN_HISTORY.md).  The lane id `te` is
// pinned to the transform's output by an asm at each site: where that pin stands matters to register allocation.
// In scope: N, m, te, ctab (ctab[k] = k_odd cot(pi k / N): even in k, 0 at k = 0 and at the Nyquist mode, which odd derivatives drop, as the
// oracle does), c1h (half the derivative factor per unit wavenumber index).  Defines ko, ke, ct, ar, ai.
            int ko, ke;
            wavenumber<N, m>(te, ko, ke);
            const float ct = ctab[ke < 0 ? -ke : ke];
            const float ar = ct * c1h, ai = (float)ko * c1h;
