// The one statement of the edit distance on the device: a column step of Myers' bit-vector algorithm in Hyyro's form for the global
// (Levenshtein) distance, unit costs, no transpositions (nltk.edit_distance's defaults).  lexicon_match.h runs it per thread on 32-bit
// words (pattern = the reading), eval_metrics.h per wave on 64-bit words (pattern = the adapted prediction, match mask = a ballot).
#pragma once

#include "common.h"

namespace pq {

// eq = the pattern positions the text character matches, top = the pattern's top bit (0 for an empty pattern: the score then stays put).
// Bits above the pattern's length never reach the ones below (carries and shifts go upwards only).
template <typename Word>
__device__ __forceinline__ void myers_step(Word eq, Word top, Word& pv, Word& mv, int& score) {
    const Word xv = eq | mv;
    const Word xh = (((eq & pv) + pv) ^ pv) | eq;
    Word ph = mv | ~(xh | pv);
    Word mh = pv & xh;
    score += (ph & top) ? 1 : 0;
    score -= (mh & top) ? 1 : 0;
    ph = (ph << 1) | Word(1);      // the DP's first row grows by one per text character
    mh <<= 1;
    pv = mh | ~(xv | ph);
    mv = ph & xv;
}

}  // namespace pq
