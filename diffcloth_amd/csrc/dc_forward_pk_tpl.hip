// CDNA4 (gfx950) forward step, packet-ELL resident variant on the packet matrix's template layout (dc_packets.h: values only, one set of
// twelve column offsets for the whole matrix — regularly numbered meshes such as a row-major grid): the instances of the kernel of
// dc_forward_pk_kernel.h whose product loop gathers with the row as an immediate offset (dc_pklib.h: PkTplRows). A translation unit of its
// own for the reason dc_forward_pk_defl.hip is one: the instances of this kernel take minutes each to compile.
#define DC_KERNEL_TU
#include "dc_forward_pk_kernel.h"

namespace dc {

hipError_t launch_pd_step_packet_template(const DevSystem &S, const DevWork &W, const FwdArgs &A, const FwdChoice &ch, int B, hipStream_t st) {
  return launch_pk_template_choice(S, W, A, ch, B, st);
}

}  // namespace dc
