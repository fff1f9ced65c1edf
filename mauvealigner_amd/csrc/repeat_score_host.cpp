// repeat_score_host.cpp -- the figures of scoreProcrastAlignment.cpp (:346-363) from the totals of mauve_repeat_score: host
// code, no context, no device.  A ratio without a denominator is 0 (the tool prints nan there).
#include "../../include/mauve_hip.h"

static double rs_ratio(int64_t a, int64_t b) { return b ? (double)a / (double)b : 0.0; }

extern "C" void mauve_repeat_score_ppv(const mauve_repeat_score_totals *t, double out[4])
{
    out[0] = rs_ratio(t->sp_truepos, t->sp_possible);
    out[1] = rs_ratio(t->sp_exact, t->sp_possible);
    out[2] = rs_ratio(t->components_hit, t->components);
    out[3] = rs_ratio(t->component_pairs_hit, t->component_pairs);
}
