// host_model.hpp -- shared host-side helpers (see host_model.cpp).
#pragma once
#include <cstdint>

#include "bath_hip.h"

namespace bath {
extern const float kNegInf;
extern const float kAminoBg[20];
bool amino_degen_has(int x, int y);
void core_transitions(const bath_hmm &h, float *tsc);
void length_model(float xsc[4][2], float nj, int L);
void match_logodds(const bath_hmm &h, int k, float sc[BATH_KP_AMINO]);

// esl_randomness_CreateFast / esl_random: x <- 69069 x + 1 on a Jenkins-mixed seed, u = x / 2^32 (the ensembles of bath_ensemble.hip,
// the sample stream of bath_calibrate.hip)
struct FastRng {
  uint32_t x;
  explicit FastRng(uint32_t seed) {
    uint32_t a = seed, b = 87654321u, c = 12345678u;
    a -= b; a -= c; a ^= (c >> 13);  b -= c; b -= a; b ^= (a << 8);   c -= a; c -= b; c ^= (b >> 13);
    a -= b; a -= c; a ^= (c >> 12);  b -= c; b -= a; b ^= (a << 16);  c -= a; c -= b; c ^= (b >> 5);
    a -= b; a -= c; a ^= (c >> 3);   b -= c; b -= a; b ^= (a << 10);  c -= a; c -= b; c ^= (b >> 15);
    x = c ? c : 42u;
  }
  static FastRng from_state(uint32_t state) { FastRng r(0); r.x = state; return r; }   // a generator carried from call to call
  double next() { x = x * 69069u + 1u; return (double)x / 4294967296.0; }
};
}  // namespace bath
