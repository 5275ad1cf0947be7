// The kernels of the second-order adjoint of the flow's step (nns_spec_ns_step_second_adjoint_f32) as a translation unit of their own, after
// the pattern of pspec_scalar_tangent.hip: the text of pspec_kernels.hip, which under this macro leaves its host entry points out and defines
// ps_second_adjoint_col_keep / ps_second_adjoint_row / ps_second_adjoint_col for the driver in pspec_kernels.o to call.  Named here and nowhere
// else: the TANGENT column kernels of stages 1-3 with a PsKeepTangent (plain, forced and LINEAR), ps_row_adj2_kernel, and ps_col_adj_kernel with
// a PsAdjSecond (stages 4 .. 0) or a PsAdjSecondLinear (stages 3-1).
#define PSPEC_SECOND_ADJOINT_TU
#include "pspec_kernels.hip"
