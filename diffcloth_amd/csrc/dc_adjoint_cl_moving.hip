// The split adjoint kernel for contexts that hold an obstacle-velocity table (dc_set_primitive_velocities): the source of dc_adjoint_cl.hip
// compiled once more as k_adjoint_step_cl_moving, which reads BwdArgs::pvel and writes dL/dw (see the note above the kernel there).
#define DC_ADJ_CL_MOVING
#include "dc_adjoint_cl.hip"
