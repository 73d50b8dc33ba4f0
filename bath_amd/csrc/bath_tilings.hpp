// bath_tilings.hpp -- the instantiation lists of the kernel templates.  Each list is stated here, once; the pick from a model length,
// the dispatch to an instantiation and the limits the entry points refuse beyond are derived from it.
#pragma once
#include <initializer_list>

// <NR, G> tile shapes of the SSV kernels: NR packed registers per lane, G lanes per target.  Every shape's cost table, kSsvRows rows of
// 16 * ((NR * G / 4 + 1) | 1) bytes, fits a workgroup's LDS (kSsvLdsMax): eight lanes end at 160 registers, 2560 nodes (ssv_table_fits)
#define BATH_SSV_SHAPES(X)                                                                                   \
  X(16, 1) X(20, 1) X(24, 1) X(28, 1) X(32, 1) X(36, 1) X(40, 1) X(44, 1) X(48, 1) X(52, 1) X(56, 1) X(60, 1) X(64, 1)     \
  X(68, 1) X(72, 1) X(76, 1)                                                                                 \
  X(160, 1) X(176, 1) X(192, 1) X(208, 1)                                                                    \
  X(40, 2) X(48, 2) X(56, 2) X(64, 2) X(72, 2) X(76, 2)                                                     \
  X(112, 2) X(128, 2) X(144, 2) X(160, 2) X(176, 2) X(192, 2) X(208, 2)                                      \
  X(112, 4) X(128, 4) X(144, 4) X(160, 4) X(176, 4) X(192, 4) X(208, 4)                                      \
  X(112, 8) X(128, 8) X(144, 8) X(160, 8)

// The other families are templates on one number, listed in ascending order: LIST(X, ...) applies X(N, ...) to every entry, handing
// on what follows X (a switch's body).
// C model nodes per lane of the frameshift kernels (bath_frameshift.hip, bath_fs_chain.hip, bath_fs_odds.hip, bath_fs5_odds.hip);
// the score-only 5-codon Forward parser of calibration (fs5_fwd_chain_kernel<C, 256, false>, launch_fs5_fwd_parser) goes over the same list
#define BATH_FS_COLUMNS(X, ...)                                                                                                          \
  X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(6, __VA_ARGS__) X(8, __VA_ARGS__) X(12, __VA_ARGS__)         \
  X(16, __VA_ARGS__) X(20, __VA_ARGS__)
// C of the wave-per-target MSV / Viterbi / Forward / Backward kernels (bath_filters.hip)
#define BATH_WAVE_COLUMNS(X, ...)                                                                                                        \
  X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(6, __VA_ARGS__) X(8, __VA_ARGS__) X(12, __VA_ARGS__)         \
  X(16, __VA_ARGS__) X(24, __VA_ARGS__) X(32, __VA_ARGS__)
// C of ssv_bath_kernel (bath_pipeline.hip): up to the longest model an OProfile holds
#define BATH_SSVB_COLUMNS(X, ...)                                                                                                        \
  X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(6, __VA_ARGS__) X(8, __VA_ARGS__) X(12, __VA_ARGS__)         \
  X(16, __VA_ARGS__) X(24, __VA_ARGS__) X(32, __VA_ARGS__) X(52, __VA_ARGS__)
// NR packed registers per lane of vit_lane_kernel (bath_viterbi.hip; bath_profile.hip picks NR from M)
#define BATH_VIT_LANE_NR(X, ...)                                                                                                         \
  X(16, __VA_ARGS__) X(32, __VA_ARGS__) X(48, __VA_ARGS__) X(64, __VA_ARGS__) X(68, __VA_ARGS__) X(72, __VA_ARGS__) X(76, __VA_ARGS__)   \
  X(80, __VA_ARGS__) X(96, __VA_ARGS__) X(112, __VA_ARGS__)
// NR of msv_lane_kernel (bath_msv_lane.hip) and msv_stage_kernel (bath_pipeline.hip): the one-lane SSV shapes of up to 152 nodes
#define BATH_MSV_LANE_NR(X, ...)                                                                                                         \
  X(16, __VA_ARGS__) X(20, __VA_ARGS__) X(24, __VA_ARGS__) X(28, __VA_ARGS__) X(32, __VA_ARGS__) X(36, __VA_ARGS__) X(40, __VA_ARGS__)   \
  X(44, __VA_ARGS__) X(48, __VA_ARGS__) X(52, __VA_ARGS__) X(56, __VA_ARGS__) X(60, __VA_ARGS__) X(64, __VA_ARGS__) X(68, __VA_ARGS__)   \
  X(72, __VA_ARGS__) X(76, __VA_ARGS__)

namespace bath {

constexpr int tiling_max(std::initializer_list<int> l) { return l.begin()[l.size() - 1]; }
constexpr int tiling_pick(std::initializer_list<int> l, int M) {
  for (int opt : l) if ((M + 63) / 64 <= opt) return opt;
  return -1;
}

}  // namespace bath

#define BATH_TILING_ENTRY(N, ...) N,
// a list's last entry
#define BATH_TILING_MAX(LIST) bath::tiling_max({LIST(BATH_TILING_ENTRY)})
// nodes per lane for an M-node model over a wave's 64 lanes: the list's smallest entry that holds them, -1 beyond its last
#define BATH_TILING_PICK(LIST, M) bath::tiling_pick({LIST(BATH_TILING_ENTRY)}, (M))
// switch (v) over a list: the body (what follows DEFAULT) sees its entry as the constant CC; DEFAULT is the branch of a v not listed
#define BATH_TILING_CASE(N, ...) case N: { constexpr int CC = N; __VA_ARGS__ } break;
#define BATH_TILING_SWITCH(LIST, v, DEFAULT, ...) switch (v) { LIST(BATH_TILING_CASE, __VA_ARGS__) default: DEFAULT }
