// The multi-speaker one-launch decode: sat_decode_persistent with a speaker struct =
// decode_persistent_kernel<false, true> / <true, true> of decode_persistent.hip, built as a
// module of their own so that the single-speaker kernels' module holds what it held before them
// (see the note above the entries there).
#define SAT_DP_SPK 1
#include "decode_persistent.hip"
