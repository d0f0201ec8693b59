// The history one-launch decode (any output width): sat_decode_persistent with a history struct,
// under either setting of the speaker and dropout structs = decode_persistent_kernel<kDrop, kSpk,
// true> of decode_persistent.hip, built as a module of their own so that the modules of the
// mel-row kernels hold what they held before these (see the note above the entries there).
#define SAT_DP_HIST 1
#include "decode_persistent.hip"
