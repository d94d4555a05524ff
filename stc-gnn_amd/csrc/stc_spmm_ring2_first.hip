// The two-ring blend on the zero initial state (stc_ring2_blend_first_f32: a cell's first time step, no H operand) as a translation unit of its
// own: stc_spmm_ring2.hip with STC_RING2_FIRST_UNIT defined compiles the R2_BLEND0 form of its kernel and that entry point alone.
#define STC_RING2_FIRST_UNIT
#include "stc_spmm_ring2.hip"
