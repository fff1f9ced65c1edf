// score_host.cpp -- the totals of scoreAlignment.cpp from the records of mauve_score_alignment: host code, no context,
// no device.  The tool visits a truth base-base pair once, from the lower sequence index (:255-260), a base-gap pair from the side that
// has the base.
#include "../../include/mauve_hip.h"

extern "C" void mauve_score_totals_from(const int64_t *records, int nseq, mauve_score_totals *out)
{
    mauve_score_totals t = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < nseq; i++)
        for (int j = 0; j < nseq; j++) {
            if (i == j) continue;
            const int64_t *s = records + ((int64_t)i * nseq + j) * MAUVE_SCORE_WORDS;
            if (i < j) { t.tp += s[0]; t.fp += s[1] + s[2]; t.fn += s[3]; t.unaligned_fn += s[3]; }
            t.fn += s[4];
            t.tn += s[5];
        }
    t.total = t.tp + t.tn + t.fp + t.fn;
    *out = t;
}
