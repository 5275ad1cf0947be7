// The kernels of the tangent of the scalar and the buoyant step (nns_spec_ns_step_scalar_tangent_f32) as a translation unit of their own:
// the text of pspec_kernels.hip, which under this macro leaves its host entry points out, names only the forms with a PsTangentScalar in
// launch_col_stage and defines ps_scalar_tangent_col / ps_scalar_tangent_row for the driver in pspec_kernels.o to call.  85 kernels that
// would otherwise lengthen the one long compilation of the library by half.
#define PSPEC_SCALAR_TANGENT_TU
#include "pspec_kernels.hip"
