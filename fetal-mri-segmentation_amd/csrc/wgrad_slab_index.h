// Index arithmetic of the kd-sharing weight-gradient kernel's slab flush (k_conv_wgrad_kd<false, true>) and of its reduction
// (k_wgrad_reduce_kd), conv3d_wgrad.hip.  Plain integer functions, callable from the host as well: tests/wgrad_slab_index_check.cpp walks
// them over real buffers under the address and undefined-behaviour sanitizers.
//
// Workspace image: ws[slab][block][tap 27][row 32 = Cout inside the block][col 32 = Cin inside the block] fp32, block = cob * ncib + cib
// (the workgroup index of the launch is slab * nblocks + block, so a workgroup's partial sums are ONE contiguous run of 27,648 floats and a
// half-wave - 32 lanes, one per col - stores 128 contiguous bytes, as the atomic flush does).
#pragma once
#include <cstdint>

#if defined(__HIP__) || defined(__HIPCC__)
#define WKS_HD __host__ __device__ __forceinline__
#else
#define WKS_HD inline
#endif

namespace wks {
constexpr int TAPS = 27, BLK = 32;
constexpr int BLOCK_FLOATS = TAPS * BLK * BLK;             // 27,648 fp32 = 110,592 bytes per (slab, block)
constexpr int BLOCK_F4 = BLOCK_FLOATS / 4;                 // 6,912 float4 columns per block (= 216 x 32: a 32-column group never straddles blocks)

// float offset of element (tap, row, col) of block `block` of slab `slab`
WKS_HD int64_t flush_index(int slab, int nblocks, int block, int tap, int row, int col) {
    return ((int64_t)slab * nblocks + block) * BLOCK_FLOATS + (tap * BLK + row) * BLK + col;
}
// slabs of one launch: one resident round of workgroups (round_wgs = 2 per CU), what the caller's workspace holds, at most one per unit.
// 0: the workspace does not hold one slab - the caller falls back to the per-kd route
WKS_HD int slab_count(int round_wgs, int nblocks, int64_t ws_bytes, int nunits) {
    int64_t n = round_wgs / nblocks;
    const int64_t fit = ws_bytes / ((int64_t)nblocks * BLOCK_FLOATS * (int64_t)sizeof(float));
    if (fit < n) n = fit;
    if (nunits < n) n = nunits;
    return n < 0 ? 0 : (int)n;
}
// reduction: float4 index in the workspace of column q (0 <= q < nblocks * BLOCK_F4) of slab `slab`
WKS_HD int64_t reduce_src4(int slab, int nblocks, int64_t q) { return (int64_t)slab * nblocks * BLOCK_F4 + q; }
// ... and the float offset in dw (row length dw_ld >= Cin) of the four elements column q sums
WKS_HD int64_t reduce_dst(int64_t q, int ncib, int Cout, int dw_ld) {
    const int block = (int)(q / BLOCK_F4), e = (int)(q % BLOCK_F4) * 4;
    const int col = e % BLK, row = (e / BLK) % BLK, tap = e / (BLK * BLK);
    const int cib = block % ncib, cob = block / ncib;
    return ((int64_t)tap * Cout + cob * BLK + row) * dw_ld + cib * BLK + col;
}
}  // namespace wks
