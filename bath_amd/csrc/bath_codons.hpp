// bath_codons.hpp -- what the host-side readers of a trace share about a (quasi-)codon of the 5-codon frameshift profile: the
// alignment renderer (bath_alidisplay.hip) and the frameshift table (bath_tophits.hip).  Host code.
#pragma once
#include <cstddef>

#include "bath_hip.h"

namespace bath {

enum { I___X = 0, I_X__, I_XX_, I_X_X, I__XX, I_XXX, I_XXx, I_XxX, I_xXX, I_xxx, I_XXxX, I_XxXX, I_xXXX, I_XXxxX, I_XxxXX, I_xxXXX };   // hmmer.h:252-270

// get_codon_index, p7_alidisplay.c:32-88
inline int codon_index(int len, const int *n) {
  bool canon = true;
  for (int q = 0; q < len; q++) canon = canon && n[q] >= 0 && n[q] < 4;
  switch (len) {
    case 1: return canon ? n[0] * 341 : 1366;
    case 2: return canon ? n[1] * 341 + n[0] * 85 + 1 : 1365;
    case 3: return canon ? n[2] * 341 + n[1] * 85 + n[0] * 21 + 2 : 1364;
    case 4: return canon ? n[3] * 341 + n[2] * 85 + n[1] * 21 + n[0] * 5 + 3 : 1365;
    default: return canon ? n[4] * 341 + n[3] * 85 + n[2] * 21 + n[1] * 5 + n[0] + 4 : 1366;
  }
}

// The profile's row of the codon <n> (len nucleotides) at node k: index into gm_fs5->codons / ->indel_pos.
inline size_t codon_row(const bath_fs_profile *gm_fs5, int k, int len, const int *n) {
  return (size_t)k * (size_t)gm_fs5->maxcodons + (size_t)codon_index(len, n);
}

// The stop-codon rule, stated once: a 3-nucleotide codon is a stop codon when the profile marks one of its nucleotides as the
// one to leave out (p7_alidisplay_fs_Create sets ad->codon = 6 on it, p7_alidisplay.c:772, :832; p7_tophits_TabularFrameshifts
// reads that mark, on match states only, for its 'S' rows, p7_tophits.c:1513).
inline bool codon3_is_stop(int indel) { return indel == I_XXx || indel == I_XxX || indel == I_xXX; }

}  // namespace bath
