// batch_limits.hpp — the sizes that the argument checks of the batch front end (batch_check.hpp) share with the kernels they guard
// (k_match.hip, k_matchf.hip, k_guided.hip). Plain C++: common.hpp includes it for the device side, the checks for the host side.
#pragma once

namespace covgpu {

// k_match.hip
constexpr int kMatchScanRows = 256;   // query rows per scan workgroup (grid = num_jobs * ceil(max query rows / 256))
// k_matchf.hip
constexpr int kMatchFloatTileRows = 128;    // query rows per scan workgroup (grid = num_jobs * ceil(max query rows / 128))
constexpr int kMatchFloatChunkRows = 64;    // train rows staged in LDS per chunk
constexpr int kMatchFloatMaxDim = 256;      // dim: a positive multiple of 4 up to this
constexpr float kMatchFloatMaxAbs = 1e18f;  // |value| bound of a descriptor entry: |x|^2 of 256 such entries stays finite in float32
// k_guided.hip: a scan tile holds at most this many points
constexpr int kGuidedScanPoints = 256;
constexpr int kGuidedListCap = 8;      // PROJECTION: entries a point keeps for the replay (more: the replay rescans)

}  // namespace covgpu
