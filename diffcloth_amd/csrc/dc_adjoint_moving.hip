// The one-workgroup adjoint kernels for contexts that hold an obstacle-velocity table (dc_set_primitive_velocities): the source of
// dc_adjoint.hip compiled once more as k_adjoint_step_moving, which reads BwdArgs::pvel and writes dL/dw (see the note at the top of that file).
#define DC_ADJ_MOVING
#include "dc_adjoint.hip"
