// Focused steps of a progressive session (rt_camera_progressive_focus): the device-side selection
// of the active pixels with the largest scores (focus.hip). A score is one fp32 per pixel - the
// session's own variance (prog_variance of the state), or a region-packed plane: an uploaded map
// or a history's variance. Sanitised as the variance filter does (not (>= 0 and finite) -> 0), a
// pixel is eligible when its score exceeds min_score; the selected set is every eligible pixel
// whose score is at least the K-th largest eligible score T, ties at T included, so it is a
// function of the scores alone whatever the order of the active list. Non-negative finite floats
// order as their uint32 bit patterns: the selection works on those. tests/focus_ref.py is the
// normative definition.
// No reference counterpart: the reference samples every pixel alike.
#pragma once

#include "progressive.hpp"

namespace rt {

// Radix select over 8-bit digits, most significant first: 4 passes of 256 bins.
constexpr int kFocusDigitBits = 8;
constexpr int kFocusBins = 1 << kFocusDigitBits;
constexpr int kFocusPasses = 32 / kFocusDigitBits;

// The selection's device words (uint32, zeroed by launch_focus_select before the kernels):
//   [0] selected count   [1] eligible count   [2] T (bit pattern; 0: nothing eligible)
//   [kFocusState + 2p, + 2p + 1]  the prefix found and the rank left before digit pass p
//   [kFocusHist + 256 p ..)       the digit histogram of pass p
constexpr int kFocusSelected = 0, kFocusEligible = 1, kFocusThreshold = 2;
constexpr int kFocusState = 4;
constexpr int kFocusHist = 16;
constexpr int kFocusWords = kFocusHist + kFocusPasses * kFocusBins;

struct FocusArgs {
    const int32_t* act;     // the session's active list
    int32_t n_act;
    uint32_t k;             // the budget K >= 1 (the kernels cap it by the eligible count)
    uint32_t min_bits;      // min_score's bit pattern (>= 0, finite)
    // the score: state (the session's variance) when plane is null, else the region-packed plane
    const ProgPix* state;
    const float* plane;
    int32_t tiles_x, w, h;  // the session's region in tiles and pixels
    int32_t x0, y0, pitch;  // the region's first pixel and the row pitch of the full-frame mask
    uint32_t* key;          // scratch, n_act entries: an eligible entry's score bits, else 0
    uint32_t* words;        // kFocusWords
    int32_t* list;          // out: the selected slots, words[kFocusSelected] of them
    uint8_t* mask;          // out, may be null: full-frame, 1 at every selected pixel (zeroed by the caller)
};

// Score pass, kFocusPasses digit passes and the compaction, queued; the host reads
// words[0 .. 3) afterwards (one copy). a.n_act > 0.
hipError_t launch_focus_select(const FocusArgs& a, hipStream_t stream);

}  // namespace rt
