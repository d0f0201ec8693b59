// The history one-launch decode (any output width): sat_decode_persistent_hist, _hist_dropout,
// _hist_spk and _hist_spk_dropout = decode_persistent_kernel<kDrop, kSpk, true> of
// decode_persistent.hip, built as a module of their own so that the modules of the mel-row
// kernels hold what they held before these (see the note above the entries there).
#define SAT_DP_HIST 1
#include "decode_persistent.hip"
