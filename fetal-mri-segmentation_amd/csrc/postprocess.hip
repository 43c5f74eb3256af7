// scipy.ndimage on the device.  First: post-processing of a predicted probability volume (reference fetal_net/postprocess.py:7-19):
//   scipy.ndimage.gaussian_filter -> "> threshold" -> binary_fill_holes -> largest connected component (scipy.ndimage.label).
// The production flow of the reference (prod/predict_nifti2.py:77-95) runs this once per stage on a whole 160x256x256-class volume; with
// the sliding-window result already in HBM it costs four small HBM-bound passes and two label-propagation loops instead of a download
// plus ~1 s of single-threaded scipy.  All kernels are word / index movers: one thread per voxel, z (contiguous) fastest.  There is one
// chain for any number of label channels, L <= 32: the masks of a voxel are the low bits of one uint32 word (the block after the
// correlate entry points); a single probability volume is that chain at L = 1.
//
// Exactness: the 1-D correlation sums in scipy's own order (centre tap first, then the symmetric pairs from the outermost inwards,
// ni_filters.c NI_Correlate1D symmetric branch) in fp64 with host-computed weights, so the smoothed volume - and therefore the
// thresholded mask - is bit-identical to scipy's; hole filling and labelling are integer algorithms with scipy's default 6-connectivity,
// and ties between equally large components go to the one scipy numbers first (smallest linear index of its first voxel).
// Second: distance_transform_edt (the distance masks of the mask-weighted loss).  Third: the B-spline resampling and the variant median
// around whole-volume prediction.  Fourth: the intensity preparation in front of the model.  Fifth, at the end of the file: scoring a
// predicted mask against the truth (overlap counts, surfaces, masked reductions over the distance field).
#include "common.h"
#include <math.h>

namespace {

__device__ __forceinline__ int reflect_idx(int i, int n) {          // scipy mode='reflect': d c b a | a b c d | d c b a
    while (i < 0 || i >= n) i = i < 0 ? -i - 1 : 2 * n - i - 1;
    return i;
}

// T = double: the post-processing volume (bit-identical to scipy).  T = float: a training patch (skimage.filters.gaussian of the
// augmentation chain, reference augment.py:113-114): the same sums in fp64, the result rounded once to the patch's fp32.
// NEAREST = scipy mode 'nearest' (a a a a | a b c d | d d d d), what skimage.filters.gaussian passes; else 'reflect'.
// ANTI = NI_Correlate1D's antisymmetric branch (weights with w[r + j] == -w[r - j]: the order-1 Gaussian of gaussian_gradient_magnitude):
// the pairs are subtracted, x[l + jj] - x[l - jj], instead of added.
// CL = a channels-last volume [X][Y][Z / L][L] (Z counts the elements of a row, L per voxel): axes 0 and 1 see rows of Z elements as
// before, axis 2 runs over the Z / L voxels of a row with an element stride of L.
template <typename T, bool NEAREST, bool ANTI = false, bool CL = false>
__global__ void k_correlate1d_sym(const T* __restrict__ src, T* __restrict__ dst, int X, int Y, int Z, int axis,
                                  const double* __restrict__ w, int radius, int L) {
#pragma clang fp contract(off)      // separately rounded multiply and add: scipy's C loop is compiled without fused operations
    const int64_t total = (int64_t)X * Y * Z;
    const int es = CL ? L : 1;
    const int n = axis == 0 ? X : (axis == 1 ? Y : Z / es);
    const int64_t stride = axis == 0 ? (int64_t)Y * Z : (axis == 1 ? Z : es);
    auto at = [&](int i) { return NEAREST ? min(max(i, 0), n - 1) : reflect_idx(i, n); };
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int z = (int)(t % Z);
        const int64_t q = t / Z;
        const int y = (int)(q % Y), x = (int)(q / Y);
        const int l = axis == 0 ? x : (axis == 1 ? y : z / es);
        const int64_t base = t - (int64_t)l * stride;
        double acc = (double)src[t] * w[radius];
        for (int jj = -radius; jj < 0; ++jj) {
            const double lo = (double)src[base + (int64_t)at(l + jj) * stride], hi = (double)src[base + (int64_t)at(l - jj) * stride];
            acc += (ANTI ? lo - hi : lo + hi) * w[jj + radius];
        }
        dst[t] = (T)acc;
    }
}

}  // namespace

extern "C" int fmri_correlate1d_f64(const double* src, double* dst, int X, int Y, int Z, int axis, const double* weights, int radius,
                                    fmri_stream_t stream) {
    if (!src || !dst || !weights || src == dst || X <= 0 || Y <= 0 || Z <= 0 || axis < 0 || axis > 2 || radius < 0) return FMRI_E_SHAPE;
    k_correlate1d_sym<double, false><<<grid_for((int64_t)X * Y * Z, 256, 8192), 256, 0, as_stream(stream)>>>(src, dst, X, Y, Z, axis, weights, radius, 1);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_correlate1d_asym_f64(const double* src, double* dst, int X, int Y, int Z, int axis, const double* weights, int radius,
                                         fmri_stream_t stream) {
    if (!src || !dst || !weights || src == dst || X <= 0 || Y <= 0 || Z <= 0 || axis < 0 || axis > 2 || radius < 0) return FMRI_E_SHAPE;
    k_correlate1d_sym<double, false, true><<<grid_for((int64_t)X * Y * Z, 256, 8192), 256, 0, as_stream(stream)>>>(src, dst, X, Y, Z, axis, weights,
                                                                                                                  radius, 1);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_correlate1d_f32(const float* src, float* dst, int X, int Y, int Z, int axis, const double* weights, int radius, int mode,
                                    fmri_stream_t stream) {
    if (!src || !dst || !weights || src == dst || X <= 0 || Y <= 0 || Z <= 0 || axis < 0 || axis > 2 || radius < 0 || (mode != 0 && mode != 1))
        return FMRI_E_SHAPE;
    const int grid = grid_for((int64_t)X * Y * Z, 256, 8192);
    if (mode == 1) k_correlate1d_sym<float, true><<<grid, 256, 0, as_stream(stream)>>>(src, dst, X, Y, Z, axis, weights, radius, 1);
    else k_correlate1d_sym<float, false><<<grid, 256, 0, as_stream(stream)>>>(src, dst, X, Y, Z, axis, weights, radius, 1);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// The clean-up for L <= 32 label channels in one pass (fetal_net.postprocess: postprocess_label_map, and postprocess_prediction at
// L = 1).  The probabilities come channels last, [X][Y][Z][L] fp64, as the tile loop leaves them.  After smoothing and "> threshold" the
// L masks of a voxel are the L low bits of one uint32 word, and every later stage works on words:
//   smoothing    k_correlate1d_sym<.., CL>: axes 0 and 1 see rows of Z * L elements, axis 2 an element stride of L - per channel the sums
//                of the plain [X][Y][Z] instantiation, bit for bit
//   threshold    a workgroup reads the 256 * L doubles of 256 voxels with coalesced loads and ORs the bits together in LDS
//   fill holes   binary_fill_holes = NOT (background reachable from outside the volume, 6-connectivity), as a flood of all channels'
//                backgrounds at once, word-wide: reached' = reached | (OR of the six neighbours' reached words & ~mask), started from
//                ~mask on the volume's border.  A voxel that takes new bits then carries them on along +z / -z inside its own row as far
//                as they go (rows are contiguous: the long axis costs one sweep instead of Z).  Several threads may add bits to one word
//                in the same sweep, so every update is an atomicOr.  `valid` (the L low bits) keeps the unused bits from ever counting
//                as background.
//   components   6-connected components by min-label propagation with root chasing.  int32 labels [L][n], channel-major: a voxel starts
//                with 1 + its index inside the channel and takes the smallest label among its neighbours of the same channel, so a
//                converged component carries 1 + the index of its first voxel - the order scipy.ndimage.label numbers the components
//                in.  One thread per voxel walks the set bits of its word, one launch per sweep and one `changed` flag for all
//                channels; a converged channel finds nothing to lower and stays as it is.  Labels are written and read only where the
//                channel's bit is set - a neighbour's bit is looked up in its word - so nothing of the L * n array is initialised or
//                read for background, and counts / best are zeroed and read only at the roots (label == own index + 1).  The count adds
//                the lanes of a wave that share a destination as one atomic; the largest component of a channel is one 64-bit max
//                over the keys (count << 32) | ~label of its roots: largest count, smallest label among equals.
//   combine      a voxel reads its word and, only for the set bits, the smoothed values: values[first argmax] or 0, one byte out
// Scratch of the whole chain at n voxels: 2 * L * n doubles (the smoothed volume and the other buffer of the passes), two uint32 [n]
// (mask / result words and `reached`), int32 [L * n] labels, int32 [L * (n + 1)] counts, uint64 [L] best.
namespace {

__global__ __launch_bounds__(256) void k_threshold_bits(const double* __restrict__ src, uint32_t* __restrict__ words, int64_t n, int L,
                                                        double thr) {
    __shared__ uint32_t w[256];
    for (int64_t base = (int64_t)blockIdx.x * 256; base < n; base += (int64_t)gridDim.x * 256) {
        w[threadIdx.x] = 0;
        __syncthreads();
        const int cnt = (int)min((int64_t)256, n - base) * L;
        const double* const p = src + base * L;
        for (int e = threadIdx.x; e < cnt; e += 256)
            if (p[e] > thr) atomicOr(&w[e / L], 1u << (e % L));
        __syncthreads();
        if (base + threadIdx.x < n) words[base + threadIdx.x] = w[threadIdx.x];
    }
}

// reached := the background bits of the words on the volume's border
__global__ void k_flood_bits_init(const uint32_t* __restrict__ mask, uint32_t* __restrict__ reached, int X, int Y, int Z, uint32_t valid) {
    const int64_t total = (int64_t)X * Y * Z;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int z = (int)(t % Z);
        const int64_t q = t / Z;
        const int y = (int)(q % Y), x = (int)(q / Y);
        const bool border = x == 0 || y == 0 || z == 0 || x == X - 1 || y == Y - 1 || z == Z - 1;
        reached[t] = border ? ~mask[t] & valid : 0u;
    }
}
// one sweep: every background bit not reached yet with a reached 6-neighbour becomes reached; then the front runs on along the z row
__global__ void k_flood_bits_sweep(const uint32_t* __restrict__ mask, uint32_t* reached, int X, int Y, int Z, uint32_t valid,
                                   int* __restrict__ changed) {
    const int64_t total = (int64_t)X * Y * Z;
    bool any = false;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t cand = ~mask[t] & valid & ~reached[t];                 // background bits not reached yet
        if (!cand) continue;
        const int z = (int)(t % Z);
        const int64_t q = t / Z;
        const int y = (int)(q % Y), x = (int)(q / Y);
        const int64_t sx = (int64_t)Y * Z;
        uint32_t nb = 0;
        if (x > 0) nb |= reached[t - sx];
        if (x < X - 1) nb |= reached[t + sx];
        if (y > 0) nb |= reached[t - Z];
        if (y < Y - 1) nb |= reached[t + Z];
        if (z > 0) nb |= reached[t - 1];
        if (z < Z - 1) nb |= reached[t + 1];
        const uint32_t add = nb & cand;
        if (!add) continue;
        atomicOr(&reached[t], add);
        any = true;
        uint32_t f = add;                                                     // the bits still running along +z, then -z
        for (int k = z + 1; k < Z; ++k) {
            f &= ~mask[t - z + k] & ~reached[t - z + k];
            if (!f) break;
            atomicOr(&reached[t - z + k], f);
        }
        f = add;
        for (int k = z - 1; k >= 0; --k) {
            f &= ~mask[t - z + k] & ~reached[t - z + k];
            if (!f) break;
            atomicOr(&reached[t - z + k], f);
        }
    }
    if (any) *changed = 1;
}
__global__ void k_fill_bits_from_reached(const uint32_t* __restrict__ reached, uint32_t* __restrict__ out, int64_t n, uint32_t valid) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) out[i] = ~reached[i] & valid;
}

__global__ void k_ccb_init(const uint32_t* __restrict__ words, int32_t* __restrict__ lab, int64_t n, uint32_t valid) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        for (uint32_t m = words[t] & valid; m; m &= m - 1) lab[(int64_t)(__ffs(m) - 1) * n + t] = (int32_t)(t + 1);
}
__global__ void k_ccb_sweep(const uint32_t* __restrict__ words, int32_t* lab, int X, int Y, int Z, uint32_t valid, int* __restrict__ changed) {
    const int64_t total = (int64_t)X * Y * Z;
    bool any = false;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t w = words[t] & valid;
        if (!w) continue;
        const int z = (int)(t % Z);
        const int64_t q = t / Z;
        const int y = (int)(q % Y), x = (int)(q / Y);
        const int64_t sx = (int64_t)Y * Z;
        const uint32_t w0 = x > 0 ? words[t - sx] : 0u, w1 = x < X - 1 ? words[t + sx] : 0u, w2 = y > 0 ? words[t - Z] : 0u,
                       w3 = y < Y - 1 ? words[t + Z] : 0u, w4 = z > 0 ? words[t - 1] : 0u, w5 = z < Z - 1 ? words[t + 1] : 0u;
        for (uint32_t todo = w & (w0 | w1 | w2 | w3 | w4 | w5); todo; todo &= todo - 1) {      // channels in which the voxel has a neighbour
            const uint32_t bit = todo & (0u - todo);
            int32_t* const lb = lab + (int64_t)(__ffs(todo) - 1) * total;
            const int32_t mine = lb[t];
            int32_t m = mine;
            auto look = [&](uint32_t wn, int64_t o) {
                if (wn & bit) {
                    const int32_t v = lb[o];
                    if (v < m) m = v;
                }
            };
            look(w0, t - sx);
            look(w1, t + sx);
            look(w2, t - Z);
            look(w3, t + Z);
            look(w4, t - 1);
            look(w5, t + 1);
            // chase the chain of representatives: the label of voxel (m - 1) is never larger than m and belongs to the same component.
            // A label is always 1 + the index of a voxel of the same component, the range test only keeps a caller's mismatched
            // words / labels inside the array
            for (int hop = 0; hop < 8 && (uint32_t)(m - 1) < (uint32_t)total; ++hop) {
                const int32_t up = lb[m - 1];
                if (up >= m) break;
                m = up;
            }
            if (m < mine && (uint32_t)(mine - 1) < (uint32_t)total && m > 0) {
                atomicMin(&lb[t], m);
                atomicMin(&lb[mine - 1], m);          // hand the better label to the old representative too (union by smaller index)
                any = true;
            }
        }
    }
    if (any) *changed = 1;
}
// roots only: counts[l][root label] = 0 and best[l] = 0 ahead of the count
__global__ void k_ccb_zero(const uint32_t* __restrict__ words, const int32_t* __restrict__ lab, int32_t* __restrict__ counts,
                           unsigned long long* __restrict__ best, int64_t n, int L, uint32_t valid) {
    if (blockIdx.x == 0 && threadIdx.x < L) best[threadIdx.x] = 0ull;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        for (uint32_t m = words[t] & valid; m; m &= m - 1) {
            const int l = __ffs(m) - 1;
            if (lab[(int64_t)l * n + t] == (int32_t)(t + 1)) counts[(int64_t)l * (n + 1) + t + 1] = 0;
        }
}
// consecutive z of one component are the common case: the lanes of the wave that share the first active lane's destination add once
__global__ void k_ccb_count(const uint32_t* __restrict__ words, const int32_t* __restrict__ lab, int32_t* __restrict__ counts, int64_t n,
                            uint32_t valid) {
    const int lane = threadIdx.x & 63;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        for (uint32_t m = words[t] & valid; m; m &= m - 1) {
            const int l = __ffs(m) - 1;
            const int32_t v = lab[(int64_t)l * n + t];
            if ((uint32_t)(v - 1) >= (uint32_t)n) continue;
            const int l0 = __builtin_amdgcn_readfirstlane(l);
            const int32_t v0 = __builtin_amdgcn_readfirstlane(v);
            const bool with_first = l == l0 && v == v0;
            const unsigned long long same = __ballot(with_first);
            if (!with_first) atomicAdd(&counts[(int64_t)l * (n + 1) + v], 1);
            else if (lane == __ffsll((long long)same) - 1) atomicAdd(&counts[(int64_t)l * (n + 1) + v], (int32_t)__popcll(same));
        }
}
// best[l] = (largest count, smallest label among equals) over channel l's roots, packed as (count << 32) | (0xffffffff - label) so that
// one 64-bit max does both
__global__ void k_ccb_best(const uint32_t* __restrict__ words, const int32_t* __restrict__ lab, const int32_t* __restrict__ counts,
                           unsigned long long* __restrict__ best, int64_t n, uint32_t valid) {
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x)
        for (uint32_t m = words[t] & valid; m; m &= m - 1) {
            const int l = __ffs(m) - 1;
            if (lab[(int64_t)l * n + t] != (int32_t)(t + 1)) continue;
            const int32_t c = counts[(int64_t)l * (n + 1) + t + 1];
            if (c > 0) atomicMax(&best[l], ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(0xffffffffu - (unsigned)(t + 1)));
        }
}
__global__ __launch_bounds__(256) void k_ccb_select(const uint32_t* __restrict__ words, const int32_t* __restrict__ lab,
                                                    const unsigned long long* __restrict__ best, uint32_t* __restrict__ out, int64_t n, int L,
                                                    uint32_t valid) {
    __shared__ int32_t want[FMRI_MAX_LABELS];
    if (threadIdx.x < FMRI_MAX_LABELS) {
        const unsigned long long b = threadIdx.x < L ? best[threadIdx.x] : 0ull;
        want[threadIdx.x] = b ? (int32_t)(0xffffffffu - (unsigned)(b & 0xffffffffull)) : -1;
    }
    __syncthreads();
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        uint32_t keep = 0;
        for (uint32_t m = words[t] & valid; m; m &= m - 1) {
            const int l = __ffs(m) - 1;
            if (lab[(int64_t)l * n + t] == want[l]) keep |= 1u << l;
        }
        out[t] = keep;
    }
}

__global__ __launch_bounds__(256) void k_label_map_bits(const uint32_t* __restrict__ words, const double* __restrict__ smoothed,
                                                        uint8_t* __restrict__ out, int64_t n, int L, uint32_t valid, FmriLabelValues V) {
    __shared__ __attribute__((aligned(4))) uint8_t vals[FMRI_MAX_LABELS];
    fmri_label_tables(V, L, vals, nullptr);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const double* const row = smoothed + t * L;
        double top = 0.0;
        int k = -1;
        for (uint32_t m = words[t] & valid; m; m &= m - 1) {                  // ascending channels, strict ">": ties stay with the lowest
            const int l = __ffs(m) - 1;
            const double v = row[l];
            if (k < 0 || v > top) { top = v; k = l; }
        }
        out[t] = k < 0 ? (uint8_t)0 : vals[k];
    }
}

inline uint32_t low_bits(int L) { return L >= 32 ? 0xffffffffu : (1u << L) - 1u; }

}  // namespace

extern "C" int fmri_correlate1d_cl_f64(const double* src, double* dst, int X, int Y, int Z, int L, int axis, const double* weights, int radius,
                                       fmri_stream_t stream) {
    if (!src || !dst || !weights || src == dst || X <= 0 || Y <= 0 || Z <= 0 || L < 1 || L > FMRI_MAX_LABELS || axis < 0 || axis > 2 ||
        radius < 0 || (int64_t)Z * L > 0x7fffffff)
        return FMRI_E_SHAPE;
    k_correlate1d_sym<double, false, false, true><<<grid_for((int64_t)X * Y * Z * L, 256, 8192), 256, 0, as_stream(stream)>>>(
        src, dst, X, Y, Z * L, axis, weights, radius, L);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_threshold_bits_f64(const double* src, uint32_t* words, int64_t n, int L, double threshold, fmri_stream_t stream) {
    if (!src || !words || n <= 0 || L < 1 || L > FMRI_MAX_LABELS) return FMRI_E_SHAPE;
    k_threshold_bits<<<grid_for(n, 256, 8192), 256, 0, as_stream(stream)>>>(src, words, n, L, threshold);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
// bit l of a word is channel l's mask, bits L..31 of the input are ignored and come out zero.  phase 0: reached := background bits on the
// volume's border; phase 1: `sweeps` propagation sweeps (sets *changed when a sweep still grew the region - the caller repeats until it
// stays 0); phase 2: out := NOT reached (the filled masks)
extern "C" int fmri_fill_holes_bits_step(const uint32_t* mask, uint32_t* reached, uint32_t* out, int X, int Y, int Z, int L, int phase,
                                         int sweeps, int* changed, fmri_stream_t stream) {
    if (!mask || !reached || X <= 0 || Y <= 0 || Z <= 0 || L < 1 || L > FMRI_MAX_LABELS) return FMRI_E_SHAPE;
    const int64_t n = (int64_t)X * Y * Z;
    const uint32_t valid = low_bits(L);
    hipStream_t st = as_stream(stream);
    const int grid = grid_for(n, 256, 8192);
    if (phase == 0) k_flood_bits_init<<<grid, 256, 0, st>>>(mask, reached, X, Y, Z, valid);
    else if (phase == 1) {
        if (!changed) return FMRI_E_SHAPE;
        for (int i = 0; i < sweeps; ++i) k_flood_bits_sweep<<<grid, 256, 0, st>>>(mask, reached, X, Y, Z, valid, changed);
    } else {
        if (!out) return FMRI_E_SHAPE;
        k_fill_bits_from_reached<<<grid, 256, 0, st>>>(reached, out, n, valid);
    }
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
// phase 0: labels := 1 + voxel index where a channel's bit is set; phase 1: `sweeps` propagation sweeps (*changed as above); phase 2:
// out := every channel's largest component (counts: int32 [L][n + 1] scratch, best: uint64 [L] scratch - zeroed here where they are
// read).  `words` is the same array in all three phases (it says where `labels` holds a label)
extern "C" int fmri_largest_components_bits_step(const uint32_t* words, int32_t* labels, int32_t* counts, unsigned long long* best,
                                                 uint32_t* out, int X, int Y, int Z, int L, int phase, int sweeps, int* changed,
                                                 fmri_stream_t stream) {
    if (!words || !labels || X <= 0 || Y <= 0 || Z <= 0 || L < 1 || L > FMRI_MAX_LABELS) return FMRI_E_SHAPE;
    const int64_t n = (int64_t)X * Y * Z;
    if (n >= 0x7fffffff) return FMRI_E_SHAPE;
    const uint32_t valid = low_bits(L);
    hipStream_t st = as_stream(stream);
    const int grid = grid_for(n, 256, 8192);
    if (phase == 0) k_ccb_init<<<grid, 256, 0, st>>>(words, labels, n, valid);
    else if (phase == 1) {
        if (!changed) return FMRI_E_SHAPE;
        for (int i = 0; i < sweeps; ++i) k_ccb_sweep<<<grid, 256, 0, st>>>(words, labels, X, Y, Z, valid, changed);
    } else {
        if (!counts || !best || !out || out == words) return FMRI_E_SHAPE;
        k_ccb_zero<<<grid, 256, 0, st>>>(words, labels, counts, best, n, L, valid);
        k_ccb_count<<<grid, 256, 0, st>>>(words, labels, counts, n, valid);
        k_ccb_best<<<grid, 256, 0, st>>>(words, labels, counts, best, n, valid);
        k_ccb_select<<<grid, 256, 0, st>>>(words, labels, best, out, n, L, valid);
    }
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_label_map_bits(const uint32_t* words, const double* smoothed, uint8_t* out, int64_t n, int L, const uint8_t* values,
                                   fmri_stream_t stream) {
    FmriLabelValues V;
    if (!words || !smoothed || !out || n <= 0 || fmri_label_values(values, L, &V) != FMRI_OK) return FMRI_E_SHAPE;
    k_label_map_bits<<<grid_for(n, 256, 8192), 256, 0, as_stream(stream)>>>(words, smoothed, out, n, L, low_bits(L), V);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// Exact Euclidean distance transform of a label volume on the device (reference fetal_net/utils/create_distance_masks.py: the distance
// masks of the mask-weighted loss, scipy.ndimage.distance_transform_edt(mask, sampling) + distance_transform_edt(1 - mask, sampling)).
// uint8 volume [X][Y][Z], z contiguous, per-axis voxel spacing, fp64: every nonzero voxel gets the distance to the nearest zero voxel,
// zero voxels get 0 (scipy's definition).
//
// Separable form on SQUARED distances: f0 = 0 on zero voxels and +inf elsewhere, then one min-plus pass per axis,
//   g(j) = min_i f(i) + (s * (i - j))^2,   axis order z, y, x;   the last pass takes the square root.
//   z (contiguous lines): a [rows x Z] tile of the mask in LDS, one forward and one backward scan per row for the nearest voxel of the
//     other class, (s_z * k)^2 written with coalesced stores.
//   y, x (strided lines): a workgroup owns the whole line for a slab of 16 contiguous z (one 128-byte line of fp64 per line element),
//     f[n][16] and w[k] = (s * k)^2 in LDS; thread (j, z) walks outwards from i = j in both directions and stops when w[k] >= best.
//     Exact: f >= 0, so no candidate beyond k can be smaller; on real labels the walk is a few tens of steps, not n.
// Arithmetic: products and sums separately rounded (fp contract off), w[k] = fl(fl(k * s) * fl(k * s)) as numpy forms it.  With unit
// spacing every squared distance is an integer below 2^53: the result equals scipy's bit for bit.  Other spacings: the two agree to a
// few ulp (another summation order, and offsets of equal true distance round differently) - tests/test_gpu_distance.py derives the bound.
//
// Two-class mode: the reference's mask is edt(m) + edt(1 - m); one summand is 0 at every voxel, so the sum is the distance to the
// nearest voxel of the OTHER class.  Both fields (f_fg: distance of the nonzero voxels to the zeros, f_bg: of the zeros to the nonzeros)
// go through the three passes of one launch each - one mask read - and the last pass computes and writes, per voxel, only the field
// of the voxel's own class.
//
// Degenerate input: a volume without a zero voxel gives +inf everywhere (there is no nearest zero; scipy returns numbers that are not
// distances there), in two-class mode a volume of one class is +inf everywhere; a volume without a nonzero voxel gives 0.
// Lines longer than EDT_LDS_MAX on an axis take k_edt_line_global for that axis: the same walk on global memory, one thread per voxel.

namespace {

constexpr int EDT_LDS_MAX = 1024;        // longest line of the LDS kernels (f[1024][16] fp64 + w[1024] = 136 KiB of the CU's 160)
constexpr int EDT_TZ = 16;               // z per slab of the strided passes: 16 fp64 = one 128-byte line
constexpr int EDT_ZTILE = 32768;         // uint16 entries of the z pass's tile (64 KiB)
constexpr int EDT_NONE = 0x7fff;         // "no voxel of the other class in this row"

__device__ __forceinline__ double edt_w(int k, double s) {
#pragma clang fp contract(off)
    const double d = (double)k * s;
    return d * d;
}

// ---- pass along z.  tile[r * pitch + z]: bit 15 = the voxel's class, bits 0-14 = distance in voxels to the nearest voxel of the other
// class in the row (EDT_NONE: there is none).  pitch (in uint16) is twice an odd number: the 32 lanes of a half wave scanning 32 rows at
// the same z touch 32 different banks.
template <bool BOTH>
__global__ __launch_bounds__(256) void k_edt_z(const uint8_t* __restrict__ mask, double* __restrict__ f_fg, double* __restrict__ f_bg,
                                               int64_t rows, int Z, double sz, int R, int pitch) {
    __shared__ uint16_t tile[EDT_ZTILE];
    const int64_t tiles = (rows + R - 1) / R;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t row0 = t * R;
        const int nr = (int)min((int64_t)R, rows - row0);
        const int64_t g0 = row0 * Z;
        const int cnt = nr * Z;
        for (int e = threadIdx.x; e < cnt; e += blockDim.x) tile[(e / Z) * pitch + e % Z] = mask[g0 + e] ? 0x8000 : 0;
        __syncthreads();
        for (int r = threadIdx.x; r < nr; r += blockDim.x) {
            uint16_t* const row = tile + r * pitch;
            int l0 = -1, l1 = -1;                        // position of the latest voxel of class 0 / 1
            for (int z = 0; z < Z; ++z) {
                const int c = row[z] >> 15;
                l0 = c ? l0 : z;
                l1 = c ? z : l1;
                const int o = c ? l0 : l1;
                row[z] = (uint16_t)((c << 15) | (o < 0 ? EDT_NONE : z - o));
            }
            l0 = l1 = -1;
            for (int z = Z - 1; z >= 0; --z) {
                const int v = row[z], c = v >> 15;
                l0 = c ? l0 : z;
                l1 = c ? z : l1;
                const int o = c ? l0 : l1;
                const int k = min(v & 0x7fff, o < 0 ? EDT_NONE : o - z);
                row[z] = (uint16_t)((c << 15) | k);
            }
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
            const int v = tile[(e / Z) * pitch + e % Z], c = v >> 15, k = v & 0x7fff;
            const double w = k == EDT_NONE ? (double)INFINITY : edt_w(k, sz);
            f_fg[g0 + e] = c ? w : 0.0;
            if (BOTH) f_bg[g0 + e] = c ? 0.0 : w;
        }
        __syncthreads();
    }
}

// the min-plus walk of one output element: f(i) at i = j, then j -+ k for k = 1, 2, ... while w(k) < best.  [lo, hi] holds every finite
// f(i) of the line (lo > hi: there is none): an element outside starts at the range's near end, nobody looks past its far end.
template <typename F, typename W>
__device__ __forceinline__ double edt_walk(int j, int lo, int hi, F f, W w) {
#pragma clang fp contract(off)
    if (lo > hi) return (double)INFINITY;
    double best = f(j);
    const int kmax = max(j - lo, hi - j);
    for (int k = max(1, max(lo - j, j - hi)); k <= kmax; ++k) {
        const double wk = w(k);
        if (wk >= best) break;
        if (j - k >= lo) best = fmin(best, f(j - k) + wk);
        if (j + k <= hi) best = fmin(best, f(j + k) + wk);
    }
    return best;
}

// ---- pass along a strided axis.  Element j of line (o, c) is at o * ostride + c + j * stride, c in [0, inner) contiguous: y: o = x,
// inner = Z, stride = Z; x: one o, inner = Y * Z, stride = Y * Z.  A workgroup takes slab after slab of EDT_TZ consecutive c and, in
// two-class mode, the two fields one after the other through the same LDS.  Work item e = j * 16 + z: a wave is 4 neighbouring j x 16 z
// (similar trip counts, conflict-free 512-byte LDS rows).  lo[z] / hi[z]: the range of finite f of line z of the slab - after the z pass
// most lines of a volume with a small label have none, and without the range every element of such a line would walk all of it.
// LAST: write sqrt; in two-class mode only where the voxel is of the field's class.
template <int NMAX, bool LAST>
__global__ __launch_bounds__(NMAX) void k_edt_line(const double* __restrict__ src0, const double* __restrict__ src1, double* __restrict__ dst0,
                                                   double* __restrict__ dst1, const uint8_t* __restrict__ mask, int nf, int64_t outer,
                                                   int64_t ostride, int64_t inner, int64_t stride, int n, double s) {
    __shared__ double f[NMAX * EDT_TZ];
    __shared__ double w[NMAX];
    __shared__ int lo[EDT_TZ], hi[EDT_TZ];
    for (int k = threadIdx.x; k < n; k += blockDim.x) w[k] = edt_w(k, s);
    const int64_t spo = (inner + EDT_TZ - 1) / EDT_TZ;
    const int cnt = n * EDT_TZ;
    for (int64_t slab = blockIdx.x; slab < outer * spo; slab += gridDim.x) {
        const int64_t c0 = (slab % spo) * EDT_TZ;
        const int64_t base = (slab / spo) * ostride + c0;
        const int tz = (int)min((int64_t)EDT_TZ, inner - c0);
        for (int fld = 0; fld < nf; ++fld) {
            const double* const src = fld ? src1 : src0;
            double* const dst = (LAST || !fld) ? dst0 : dst1;
            __syncthreads();                                   // w is written / the previous round's reads of f, lo, hi are done
            if (threadIdx.x < EDT_TZ) lo[threadIdx.x] = n, hi[threadIdx.x] = -1;
            int mylo = n, myhi = -1;                           // blockDim is a multiple of 16: a thread stays on one z, its j ascend
            for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
                const int z = e % EDT_TZ, j = e / EDT_TZ;
                if (z >= tz) continue;
                const double v = src[base + (int64_t)j * stride + z];
                f[e] = v;
                if (v < (double)INFINITY) mylo = min(mylo, j), myhi = j;
            }
            __syncthreads();
            if (myhi >= 0) atomicMin(&lo[threadIdx.x % EDT_TZ], mylo), atomicMax(&hi[threadIdx.x % EDT_TZ], myhi);
            __syncthreads();
            for (int e = threadIdx.x; e < cnt; e += blockDim.x) {
                const int z = e % EDT_TZ, j = e / EDT_TZ;
                if (z >= tz) continue;
                const int64_t at = base + (int64_t)j * stride + z;
                if (LAST && nf == 2 && (mask[at] != 0) != (fld == 0)) continue;
                const double best = edt_walk(j, lo[z], hi[z], [&](int i) { return f[i * EDT_TZ + z]; }, [&](int k) { return w[k]; });
                dst[at] = LAST ? sqrt(best) : best;
            }
        }
    }
}

// ---- the slow, always applicable pass: one thread per voxel, the same walk on global memory.  FIRST: the source is the mask itself
// (field 0: f0 = mask ? inf : 0, field 1: the complement).
template <bool FIRST, bool LAST>
__global__ void k_edt_line_global(const void* __restrict__ src, double* __restrict__ dst, const uint8_t* __restrict__ mask, int fld, int two,
                                  int X, int Y, int Z, int axis, double s) {
    const int64_t total = (int64_t)X * Y * Z;
    const int n = axis == 0 ? X : (axis == 1 ? Y : Z);
    const int64_t stride = axis == 0 ? (int64_t)Y * Z : (axis == 1 ? Z : 1);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        if (LAST && two && (mask[t] != 0) != (fld == 0)) continue;
        const int64_t q = t / Z;
        const int j = axis == 0 ? (int)(q / Y) : (axis == 1 ? (int)(q % Y) : (int)(t % Z));
        const int64_t base = t - (int64_t)j * stride;
        const double best = edt_walk(j, 0, n - 1,
            [&](int i) {
                if (FIRST) return ((((const uint8_t*)src)[base + (int64_t)i * stride] != 0) != (fld != 0)) ? (double)INFINITY : 0.0;
                return ((const double*)src)[base + (int64_t)i * stride];
            },
            [&](int k) { return edt_w(k, s); });
        dst[t] = LAST ? sqrt(best) : best;
    }
}

template <bool LAST>
void launch_line(const double* s0, const double* s1, double* d0, double* d1, const uint8_t* mask, int nf, int X, int Y, int Z, int axis, double s,
                 hipStream_t st) {
    const int n = axis == 0 ? X : Y;
    const int64_t total = (int64_t)X * Y * Z;
    if (n > EDT_LDS_MAX) {
        const int grid = grid_for(total, 256, 8192);
        k_edt_line_global<false, LAST><<<grid, 256, 0, st>>>(s0, d0, mask, 0, nf == 2, X, Y, Z, axis, s);
        if (nf == 2) k_edt_line_global<false, LAST><<<grid, 256, 0, st>>>(s1, LAST ? d0 : d1, mask, 1, 1, X, Y, Z, axis, s);
        return;
    }
    const int64_t outer = axis == 0 ? 1 : X, inner = axis == 0 ? (int64_t)Y * Z : Z, stride = inner, ostride = (int64_t)Y * Z;
    const int64_t slabs = outer * ceil_div64(inner, EDT_TZ);
    const int grid = (int)(slabs < 65536 ? slabs : 65536);
    if (n <= 256) k_edt_line<256, LAST><<<grid, 256, 0, st>>>(s0, s1, d0, d1, mask, nf, outer, ostride, inner, stride, n, s);
    else if (n <= 512) k_edt_line<512, LAST><<<grid, 512, 0, st>>>(s0, s1, d0, d1, mask, nf, outer, ostride, inner, stride, n, s);
    else k_edt_line<1024, LAST><<<grid, 1024, 0, st>>>(s0, s1, d0, d1, mask, nf, outer, ostride, inner, stride, n, s);
}

// the three passes; a0/a1 = the fields after z, b0/b1 after y (two-class: a0 = out, the rest scratch; one class: a0 = out, b0 = scratch)
int edt_run(const uint8_t* mask, double* out, double* scratch, int X, int Y, int Z, double sx, double sy, double sz, int nf, hipStream_t st) {
    const int64_t total = (int64_t)X * Y * Z, rows = (int64_t)X * Y;
    double* const a0 = out;
    double* const a1 = nf == 2 ? scratch : nullptr;
    double* const b0 = nf == 2 ? scratch + total : scratch;
    double* const b1 = nf == 2 ? scratch + 2 * total : nullptr;
    if (Z > EDT_LDS_MAX) {
        const int grid = grid_for(total, 256, 8192);
        k_edt_line_global<true, false><<<grid, 256, 0, st>>>(mask, a0, mask, 0, nf == 2, X, Y, Z, 2, sz);
        if (nf == 2) k_edt_line_global<true, false><<<grid, 256, 0, st>>>(mask, a1, mask, 1, 1, X, Y, Z, 2, sz);
    } else {
        int pitch = (Z + 1) & ~1;
        if (!((pitch >> 1) & 1)) pitch += 2;
        int R = EDT_ZTILE / pitch;
        if (R > 256) R = 256;
        const int64_t tiles = ceil_div64(rows, R);
        const int grid = (int)(tiles < 65536 ? tiles : 65536);
        if (nf == 2) k_edt_z<true><<<grid, 256, 0, st>>>(mask, a0, a1, rows, Z, sz, R, pitch);
        else k_edt_z<false><<<grid, 256, 0, st>>>(mask, a0, nullptr, rows, Z, sz, R, pitch);
    }
    FMRI_LAUNCH_CHECK();
    launch_line<false>(a0, a1, b0, b1, mask, nf, X, Y, Z, 1, sy, st);
    FMRI_LAUNCH_CHECK();
    launch_line<true>(b0, b1, out, nullptr, mask, nf, X, Y, Z, 0, sx, st);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

bool edt_args_ok(const uint8_t* mask, const double* out, const double* scratch, int X, int Y, int Z, double sx, double sy, double sz) {
    return mask && out && scratch && X > 0 && Y > 0 && Z > 0 && sx > 0 && sy > 0 && sz > 0 && isfinite(sx) && isfinite(sy) && isfinite(sz);
}

}  // namespace

extern "C" int fmri_edt_lds_max_line(void) { return EDT_LDS_MAX; }

extern "C" int fmri_edt_u8(const uint8_t* mask, double* out, double* scratch, int X, int Y, int Z, double sx, double sy, double sz,
                           fmri_stream_t stream) {
    if (!edt_args_ok(mask, out, scratch, X, Y, Z, sx, sy, sz)) return FMRI_E_SHAPE;
    return edt_run(mask, out, scratch, X, Y, Z, sx, sy, sz, 1, as_stream(stream));
}

extern "C" int fmri_edt_two_class_u8(const uint8_t* mask, double* out, double* scratch, int X, int Y, int Z, double sx, double sy, double sz,
                                     fmri_stream_t stream) {
    if (!edt_args_ok(mask, out, scratch, X, Y, Z, sx, sy, sz)) return FMRI_E_SHAPE;
    return edt_run(mask, out, scratch, X, Y, Z, sx, sy, sz, 2, as_stream(stream));
}

// ---------------------------------------------------------------------------------------------------------------------------------------
// scipy.ndimage's quadratic / cubic B-spline resampling on the device, fp64 (ndimage.zoom / rotate / affine_transform with
// mode='constant': the resolution change and its inverse of fetal_net.pipeline.Zoom, the in-plane rotations of predict_augment), and the
// voxel-wise median over a stack of test-time variants.  The arithmetic is scipy's C code restated (ni_splines.c, ni_interpolation.c),
// every product and sum separately rounded:
//   prefilter (spline_filter1d, mode 'mirror' - what scipy filters with for 'constant'): one pole z = sqrt(8) - 3 (order 2) or
//     sqrt(3) - 2 (order 3); c *= (1 - z)(1 - 1/z); c[0] = (c[0] + z^(n-1) c[n-1] + sum_{i=1..n-2} z^i (c[i] + z^(n-1) c[n-1-i])) /
//     (1 - z^(2n-2)); c[i] += z c[i-1]; c[n-1] = (z c[n-2] + c[n-1]) z / (z^2 - 1); c[i] = z (c[i+1] - c[i]).  One lane owns one line.
//     Strided axes: consecutive lanes sit on consecutive z, so every step of the recursion reads and writes a coalesced row.  The
//     contiguous axis: a [rows x Z] tile in LDS (coalesced both ways), one lane per row; the row pitch is an odd number of doubles, so
//     the 32 lanes of a half wave, all at the same z of 32 rows, hit 32 different 8-byte bank pairs.  The tile is 72 KiB: two workgroups
//     per CU.  A contiguous line longer than SPL_LDS_MAX runs the strided kernel with stride 1 (uncoalesced, same result).
//   interpolation: input coordinate c_a = ((M_a0 i + M_a1 j) + M_a2 k) + t_a; a coordinate outside [0, n_a - 1] on any axis gives cval
//     (it decides whole voxels - a fused multiply-add here would move voxels in and out); footprint of order + 1 taps per axis from
//     floor(c) - order/2 (odd order) or floor(c + 0.5) - order/2 (even), indices beyond the edge mirrored about the end samples, scipy's
//     weights; value = sum over the footprint, last axis fastest, of ((v w0) w1) w2.  The spline order is a template argument per axis:
//     weights and indices live in registers (no scratch memory).  Lanes run along the contiguous output axis; neighbouring outputs share
//     their footprints, so most of the up to 64 gathers per output hit in cache.
//   median: one lane per voxel, the K <= 64 values in registers (padded with +inf to 8 / 16 / 32 / 64), a fully unrolled bitonic
//     network, the middle element or the two middle elements added and halved (np.median).  NaN is not specified.

namespace {

constexpr int SPL_LDS_MAX = 1024;        // longest contiguous line of the LDS kernel (at least 8 rows per tile)
constexpr int SPL_TILE = 9216;           // doubles in the tile: 72 KiB

// the recursion on one line.  first(i): element i as stored, times the gain (the gain pass of scipy folded into the first read);
// get(i) / put(i, v): element i after it has been rewritten.  n >= 2.
template <typename First, typename Get, typename Put>
__device__ __forceinline__ void spline_line(int n, double z, double zn1, First first, Get get, Put put) {
#pragma clang fp contract(off)
    double c0 = first(0) + zn1 * first(n - 1);
    double zi = z;
    for (int i = 1; i < n - 1 && zi != 0.0; ++i) {          // z^i underflows to 0 after some hundred elements: the rest adds nothing
        c0 += zi * (first(i) + zn1 * first(n - 1 - i));
        zi *= z;
    }
    c0 /= 1.0 - zn1 * zn1;
    put(0, c0);
    double prev = c0, prev2 = c0;
    for (int i = 1; i < n; ++i) {
        prev2 = prev;
        prev = first(i) + z * prev;
        put(i, prev);
    }
    double next = (z * prev2 + prev) * z / (z * z - 1.0);
    put(n - 1, next);
    for (int i = n - 2; i >= 0; --i) {
        next = z * (next - get(i));
        put(i, next);
    }
}

// line t of `lines`: element j at (t / inner) * ostride + t % inner + j * stride
__global__ __launch_bounds__(64) void k_spline_lines(double* __restrict__ vol, int64_t lines, int64_t inner, int64_t ostride, int64_t stride, int n,
                                                     double z, double gain, double zn1) {
#pragma clang fp contract(off)
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < lines; t += (int64_t)gridDim.x * blockDim.x) {
        double* const p = vol + (t / inner) * ostride + t % inner;
        spline_line(n, z, zn1, [&](int i) { return p[i * stride] * gain; }, [&](int i) { return p[i * stride]; },
                    [&](int i, double v) { p[i * stride] = v; });
    }
}

__global__ __launch_bounds__(256) void k_spline_z(double* __restrict__ vol, int64_t rows, int Z, int R, int pitch, double z, double gain,
                                                  double zn1) {
#pragma clang fp contract(off)
    __shared__ double tile[SPL_TILE];
    const int64_t tiles = (rows + R - 1) / R;
    for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int64_t row0 = t * R;
        const int nr = (int)min((int64_t)R, rows - row0);
        const int64_t g0 = row0 * Z;
        const int cnt = nr * Z;
        for (int e = threadIdx.x; e < cnt; e += blockDim.x) tile[(e / Z) * pitch + e % Z] = vol[g0 + e] * gain;
        __syncthreads();
        for (int r = threadIdx.x; r < nr; r += blockDim.x) {
            double* const row = tile + r * pitch;
            spline_line(Z, z, zn1, [&](int i) { return row[i]; }, [&](int i) { return row[i]; }, [&](int i, double v) { row[i] = v; });
        }
        __syncthreads();
        for (int e = threadIdx.x; e < cnt; e += blockDim.x) vol[g0 + e] = tile[(e / Z) * pitch + e % Z];
        __syncthreads();
    }
}

struct Affine12 { double m[12]; };

// footprint of one axis: ORDER + 1 taps, first index and weights as scipy forms them, indices mirrored into [0, n)
template <int ORDER>
__device__ __forceinline__ void spline_taps(double c, int n, int (&idx)[4], double (&w)[4]) {
#pragma clang fp contract(off)
    const double f = (ORDER & 1) ? floor(c) : floor(c + 0.5);
    const double y = c - f;
    if (ORDER == 0) {
        w[0] = 1.0;
    } else if (ORDER == 1) {
        w[0] = 1.0 - y;
        w[1] = y;
    } else if (ORDER == 2) {
        w[0] = 0.5 * ((0.5 - y) * (0.5 - y));
        w[1] = 0.75 - y * y;
        w[2] = 0.5 * ((0.5 + y) * (0.5 + y));
    } else {
        const double u = 1.0 - y;
        w[0] = u * u * u / 6.0;
        w[1] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
        w[2] = (u * u * (u - 2.0) * 3.0 + 4.0) / 6.0;
        w[3] = y * y * y / 6.0;
    }
    const int start = (int)f - ORDER / 2;
    const int s2 = 2 * n - 2;
#pragma unroll
    for (int a = 0; a <= ORDER; ++a) {
        int m = 0;
        if (n > 1) {
            m = (start + a) % s2;
            m = m < 0 ? m + s2 : m;
            m = m >= n ? s2 - m : m;
        }
        idx[a] = m;
    }
}

template <int O0, int O1, int O2>
__global__ __launch_bounds__(256) void k_spline_affine(const double* __restrict__ coef, int X, int Y, int Z, Affine12 A, double* __restrict__ out,
                                                       int NX, int NY, int NZ, double cval) {
#pragma clang fp contract(off)
    const int64_t total = (int64_t)NX * NY * NZ;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t q = t / NZ;
        const double k = (double)(int)(t % NZ), j = (double)(int)(q % NY), i = (double)(int)(q / NY);
        const double c0 = ((A.m[0] * i + A.m[1] * j) + A.m[2] * k) + A.m[3];
        const double c1 = ((A.m[4] * i + A.m[5] * j) + A.m[6] * k) + A.m[7];
        const double c2 = ((A.m[8] * i + A.m[9] * j) + A.m[10] * k) + A.m[11];
        if (c0 < 0.0 || c0 > (double)(X - 1) || c1 < 0.0 || c1 > (double)(Y - 1) || c2 < 0.0 || c2 > (double)(Z - 1)) {
            out[t] = cval;
            continue;
        }
        int i0[4], i1[4], i2[4];
        double w0[4], w1[4], w2[4];
        spline_taps<O0>(c0, X, i0, w0);
        spline_taps<O1>(c1, Y, i1, w1);
        spline_taps<O2>(c2, Z, i2, w2);
        double acc = 0.0;
#pragma unroll
        for (int a = 0; a <= O0; ++a)
#pragma unroll
            for (int b = 0; b <= O1; ++b) {
                const double* const line = coef + ((int64_t)i0[a] * Y + i1[b]) * Z;
#pragma unroll
                for (int c = 0; c <= O2; ++c) {
                    double v = line[i2[c]];
                    if (O0 > 0) v *= w0[a];
                    if (O1 > 0) v *= w1[b];
                    if (O2 > 0) v *= w2[c];
                    acc += v;
                }
            }
        out[t] = acc;
    }
}

struct AffineLaunch {
    const double* coef;
    int X, Y, Z;
    Affine12 A;
    double* out;
    int NX, NY, NZ;
    double cval;
    hipStream_t st;
};
template <int O0, int O1, int O2>
void affine_go(const AffineLaunch& a) {
    k_spline_affine<O0, O1, O2><<<grid_for((int64_t)a.NX * a.NY * a.NZ, 256, 65536), 256, 0, a.st>>>(a.coef, a.X, a.Y, a.Z, a.A, a.out, a.NX, a.NY,
                                                                                                     a.NZ, a.cval);
}
template <int O0, int O1>
void affine_pick2(int o2, const AffineLaunch& a) {
    switch (o2) {
        case 0: affine_go<O0, O1, 0>(a); break;
        case 1: affine_go<O0, O1, 1>(a); break;
        case 2: affine_go<O0, O1, 2>(a); break;
        default: affine_go<O0, O1, 3>(a); break;
    }
}
template <int O0>
void affine_pick1(int o1, int o2, const AffineLaunch& a) {
    switch (o1) {
        case 0: affine_pick2<O0, 0>(o2, a); break;
        case 1: affine_pick2<O0, 1>(o2, a); break;
        case 2: affine_pick2<O0, 2>(o2, a); break;
        default: affine_pick2<O0, 3>(o2, a); break;
    }
}

// compare-exchange network on KB registers; K of them hold values, the rest +inf
template <int KB>
__global__ __launch_bounds__(256) void k_median_stack(const double* __restrict__ stack, int K, int64_t n, double* __restrict__ out) {
#pragma clang fp contract(off)
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        double v[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) v[k] = k < K ? stack[(int64_t)k * n + t] : (double)INFINITY;
#pragma unroll
        for (int size = 2; size <= KB; size <<= 1)
#pragma unroll
            for (int d = size >> 1; d > 0; d >>= 1)
#pragma unroll
                for (int a = 0; a < KB; ++a) {
                    const int b = a ^ d;
                    if (b > a) {
                        const double lo = fmin(v[a], v[b]), hi = fmax(v[a], v[b]);
                        const bool up = (a & size) == 0;
                        v[a] = up ? lo : hi;
                        v[b] = up ? hi : lo;
                    }
                }
        double m0 = 0.0, m1 = 0.0;
        const int k0 = (K - 1) / 2, k1 = K / 2;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            m0 = k == k0 ? v[k] : m0;
            m1 = k == k1 ? v[k] : m1;
        }
        out[t] = (m0 + m1) / 2.0;
    }
}

// ---- agreement of the K test-time variants: ONE pass over the stack [K][nvox][C] that writes the median of k_median_stack (same network,
// same bits) and, from the same registers, the variants' mean, population variance, the binary entropy of the mean, the share of variants
// on the other side of the threshold than the median, and the set sizes |M|, |V_k|, |V_k & M| per channel (M = median > thr, V_k = v_k >
// thr).  Mean, variance terms and the K-bit mask of v_k > thr are taken BEFORE the network reorders the registers.  fp64, contraction off,
// one rounding per written operation: numpy in the same order gives the same bits (the entropy up to the two log2).
//   C == 1: a thread takes VEC consecutive voxels; VEC = 2 (16-byte loads and stores) where every pointer and the row pitch allow it and
//           2 * KB values fit the registers (KB <= 16), else 1.
//   C  > 1: a thread takes ONE voxel and walks its C channels, so at every step all 64 lanes of a wave hold the same channel and one
//           ballot per counter serves it exactly as for C == 1 (a thread per element would mix channels inside a wave and need a
//           per-lane scatter into the counters); a wave's 8-byte loads of one step are C * 8 bytes apart and the C steps together use
//           every byte of the lines they touch.
// Counts: per counter one __ballot + popcount per wave (a 64-bit mask), lane s of the wave keeps counter s of the element in a register,
// one LDS atomic per lane adds them to the workgroup's table, and the workgroup leaves with one 64-bit atomicAdd per non-zero counter.
// The loop bounds are the same for every lane of a wave (lanes past the end are switched off by `live`), so every ballot is taken by the
// full wave.  A workgroup counts fewer than 2^32 elements: the grid-stride loop gives it at most n / gridDim of them.
// FULL = (K == KB): the instantiation of the full network (the eight flips), in which no `k < K` is left to evaluate.
constexpr int TTA_CUS = 256;
// workgroups per CU the grid is capped at, by KB: all of them resident at once (tools/kernel_resources.py: 76-122 registers at KB 8 and
// 16, 146 at 32, 243-250 at 64), so the grid-stride loop has no second, thinner round of workgroups; 6 or 8 per CU measured no faster
constexpr int tta_blocks_per_cu(int KB) { return KB <= 16 ? 4 : (KB == 32 ? 2 : 1); }
constexpr int TTA_MAX_C = 16;

template <int KB>
__device__ __forceinline__ void tta_sort(double (&v)[KB]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int size = 2; size <= KB; size <<= 1)
#pragma unroll
        for (int d = size >> 1; d > 0; d >>= 1)
#pragma unroll
            for (int a = 0; a < KB; ++a) {
                const int b = a ^ d;
                if (b > a) {
                    const double lo = fmin(v[a], v[b]), hi = fmax(v[a], v[b]);
                    const bool up = (a & size) == 0;
                    v[a] = up ? lo : hi;
                    v[b] = up ? hi : lo;
                }
            }
}

struct TtaOut {
    double *median, *mean, *variance, *entropy, *disagreement;
};

template <int KB, int VEC, bool FULL>
__global__ __launch_bounds__(256) void k_tta_agreement(const double* __restrict__ stack, int K_, int64_t nvox, int C, double thr, TtaOut o,
                                                       unsigned long long* __restrict__ counts) {
#pragma clang fp contract(off)
    const int K = FULL ? KB : K_;                             // FULL: K == KB, every `k < K` below folds away
    constexpr int SLOTS = 2 * KB + 1;                         // register slots of a wave: 0 = |M|, 1 + k = |V_k|, 1 + KB + k = |V_k & M|
    constexpr int NACC = (SLOTS + 63) / 64;
    __shared__ unsigned int s_cnt[TTA_MAX_C * 129];
    const int NC = 2 * K + 1;
    const int lane = threadIdx.x & 63;
    if (counts) {
        for (int i = threadIdx.x; i < C * NC; i += 256) s_cnt[i] = 0u;
        __syncthreads();
    }
    const int64_t n = nvox * C;                               // pitch of one variant
    const int64_t units = C == 1 ? nvox / VEC : nvox;
    const bool need_mu = o.mean || o.variance || o.entropy;
    const unsigned long long valid = K == 64 ? ~0ull : (1ull << K) - 1ull;
    const double dK = (double)K;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < units; base += (int64_t)gridDim.x * 256) {
        const int64_t u = base + threadIdx.x;
        const bool live = u < units;
        for (int c = 0; c < C; ++c) {
            const int64_t e = C == 1 ? u * VEC : u * C + c;   // first element of this thread's step
            double v[VEC][KB];
#pragma unroll
            for (int k = 0; k < KB; ++k) {
                if constexpr (VEC == 2) {
                    double2 two = make_double2(0.0, 0.0);
                    if (k < K && live) two = *reinterpret_cast<const double2*>(stack + (int64_t)k * n + e);
                    v[0][k] = k < K ? two.x : (double)INFINITY;
                    v[VEC - 1][k] = k < K ? two.y : (double)INFINITY;
                } else {
                    v[0][k] = k < K ? (live ? stack[(int64_t)k * n + e] : 0.0) : (double)INFINITY;
                }
            }
            unsigned int acc[NACC];
#pragma unroll
            for (int i = 0; i < NACC; ++i) acc[i] = 0u;
            double r_med[VEC], r_mu[VEC], r_var[VEC], r_ent[VEC], r_dis[VEC];
#pragma unroll
            for (int j = 0; j < VEC; ++j) {
                double mu = 0.0, var = 0.0;
                if (need_mu) {
                    double s = v[j][0];
#pragma unroll
                    for (int k = 1; k < KB; ++k) s = k < K ? s + v[j][k] : s;
                    mu = s / dK;
                }
                if (o.variance) {
                    double q = 0.0;
#pragma unroll
                    for (int k = 0; k < KB; ++k) {
                        const double dv = v[j][k] - mu;
                        q = k < K ? q + dv * dv : q;
                    }
                    var = q / dK;
                }
                unsigned long long bits = 0ull;
#pragma unroll
                for (int k = 0; k < KB; ++k) bits |= v[j][k] > thr ? 1ull << k : 0ull;
                bits &= valid;                                // the +inf padding is no variant
                tta_sort<KB>(v[j]);
                double m0 = 0.0, m1 = 0.0;
                const int k0 = (K - 1) / 2, k1 = K / 2;
#pragma unroll
                for (int k = 0; k < KB; ++k) {
                    m0 = k == k0 ? v[j][k] : m0;
                    m1 = k == k1 ? v[j][k] : m1;
                }
                const double med = (m0 + m1) / 2.0;
                const bool m = med > thr;
                r_med[j] = med;
                r_mu[j] = mu;
                r_var[j] = var;
                r_ent[j] = 0.0;
                if (o.entropy) {
                    const double p = fmin(fmax(mu, 0.0), 1.0);
                    if (p > 0.0 && p < 1.0) {
                        const double q = 1.0 - p;
                        r_ent[j] = -(p * log2(p) + q * log2(q));
                    }
                }
                r_dis[j] = (double)__popcll(m ? ~bits & valid : bits) / dK;
                if (counts) {
                    const unsigned long long M = __ballot(live && m);
                    acc[0] += lane == 0 ? (unsigned int)__popcll(M) : 0u;
#pragma unroll
                    for (int k = 0; k < KB; ++k)
                        if (k < K) {
                            const unsigned long long Vk = __ballot(live && ((bits >> k) & 1ull) != 0ull);
                            const int sv = 1 + k, si = 1 + KB + k;
                            acc[sv >> 6] += lane == (sv & 63) ? (unsigned int)__popcll(Vk) : 0u;
                            acc[si >> 6] += lane == (si & 63) ? (unsigned int)__popcll(Vk & M) : 0u;
                        }
                }
            }
            if (live) {
                if constexpr (VEC == 2) {
                    *reinterpret_cast<double2*>(o.median + e) = make_double2(r_med[0], r_med[VEC - 1]);
                    if (o.mean) *reinterpret_cast<double2*>(o.mean + e) = make_double2(r_mu[0], r_mu[VEC - 1]);
                    if (o.variance) *reinterpret_cast<double2*>(o.variance + e) = make_double2(r_var[0], r_var[VEC - 1]);
                    if (o.entropy) *reinterpret_cast<double2*>(o.entropy + e) = make_double2(r_ent[0], r_ent[VEC - 1]);
                    if (o.disagreement) *reinterpret_cast<double2*>(o.disagreement + e) = make_double2(r_dis[0], r_dis[VEC - 1]);
                } else {
                    o.median[e] = r_med[0];
                    if (o.mean) o.mean[e] = r_mu[0];
                    if (o.variance) o.variance[e] = r_var[0];
                    if (o.entropy) o.entropy[e] = r_ent[0];
                    if (o.disagreement) o.disagreement[e] = r_dis[0];
                }
            }
            if (counts) {
#pragma unroll
                for (int i = 0; i < NACC; ++i) {
                    const int s = lane + 64 * i;              // register slot -> counter: the slots are laid out for KB, the table for K
                    const int k = s == 0 ? 0 : (s <= KB ? s - 1 : s - 1 - KB);
                    const int idx = s == 0 ? 0 : (s <= KB ? s : s - KB + K);
                    if (s < SLOTS && k < K && acc[i] != 0u) atomicAdd(&s_cnt[c * NC + idx], acc[i]);
                }
            }
        }
    }
    if (counts) {
        __syncthreads();
        for (int i = threadIdx.x; i < C * NC; i += 256)
            if (s_cnt[i] != 0u) atomicAdd(&counts[i], (unsigned long long)s_cnt[i]);
    }
}

template <int KB, int VEC>
void tta_go(const double* stack, int K, int64_t nvox, int C, double thr, const TtaOut& o, unsigned long long* counts, hipStream_t st) {
    const int64_t units = C == 1 ? nvox / VEC : nvox;
    const int grid = grid_for(units, 256, TTA_CUS * tta_blocks_per_cu(KB));
    if (K == KB) k_tta_agreement<KB, VEC, true><<<grid, 256, 0, st>>>(stack, K, nvox, C, thr, o, counts);
    else k_tta_agreement<KB, VEC, false><<<grid, 256, 0, st>>>(stack, K, nvox, C, thr, o, counts);
}

}  // namespace

extern "C" int fmri_spline_lds_max_line(void) { return SPL_LDS_MAX; }

extern "C" int fmri_spline_filter1d_f64(double* vol, int X, int Y, int Z, int axis, int order, fmri_stream_t stream) {
    if (!vol || X <= 0 || Y <= 0 || Z <= 0 || axis < 0 || axis > 2 || (order != 2 && order != 3)) return FMRI_E_SHAPE;
    const int n = axis == 0 ? X : (axis == 1 ? Y : Z);
    if (n < 2) return FMRI_OK;                               // scipy leaves a line of one sample as it is
    const double z = order == 2 ? sqrt(8.0) - 3.0 : sqrt(3.0) - 2.0;
    const double gain = (1.0 - z) * (1.0 - 1.0 / z), zn1 = pow(z, (double)(n - 1));
    hipStream_t st = as_stream(stream);
    const int64_t yz = (int64_t)Y * Z, rows = (int64_t)X * Y;
    if (axis == 2 && Z <= SPL_LDS_MAX) {
        const int pitch = Z | 1;
        int R = SPL_TILE / pitch;
        if (R > 256) R = 256;
        const int64_t tiles = ceil_div64(rows, R);
        k_spline_z<<<(int)(tiles < 65536 ? tiles : 65536), 256, 0, st>>>(vol, rows, Z, R, pitch, z, gain, zn1);
    } else {
        const int64_t lines = axis == 0 ? yz : (axis == 1 ? (int64_t)X * Z : rows);
        const int64_t inner = axis == 0 ? yz : (axis == 1 ? Z : 1), ostride = axis == 2 ? Z : yz, stride = axis == 0 ? yz : (axis == 1 ? Z : 1);
        k_spline_lines<<<grid_for(lines, 64, 65536), 64, 0, st>>>(vol, lines, inner, ostride, stride, n, z, gain, zn1);
    }
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_spline_affine_f64(const double* coef, int X, int Y, int Z, const double* affine12_host, const int* orders3, double* out,
                                      int NX, int NY, int NZ, double cval, fmri_stream_t stream) {
    if (!coef || !affine12_host || !orders3 || !out || coef == out || X <= 0 || Y <= 0 || Z <= 0 || NX <= 0 || NY <= 0 || NZ <= 0)
        return FMRI_E_SHAPE;
    for (int a = 0; a < 3; ++a)
        if (orders3[a] < 0 || orders3[a] > 3) return FMRI_E_SHAPE;
    AffineLaunch a{coef, X, Y, Z, {}, out, NX, NY, NZ, cval, as_stream(stream)};
    for (int e = 0; e < 12; ++e) a.A.m[e] = affine12_host[e];
    switch (orders3[0]) {
        case 0: affine_pick1<0>(orders3[1], orders3[2], a); break;
        case 1: affine_pick1<1>(orders3[1], orders3[2], a); break;
        case 2: affine_pick1<2>(orders3[1], orders3[2], a); break;
        default: affine_pick1<3>(orders3[1], orders3[2], a); break;
    }
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_median_stack_f64(const double* stack, int K, int64_t n, double* out, fmri_stream_t stream) {
    if (!stack || !out || K < 1 || K > 64 || n <= 0) return FMRI_E_SHAPE;
    hipStream_t st = as_stream(stream);
    const int grid = grid_for(n, 256, 65536);
    if (K <= 8) k_median_stack<8><<<grid, 256, 0, st>>>(stack, K, n, out);
    else if (K <= 16) k_median_stack<16><<<grid, 256, 0, st>>>(stack, K, n, out);
    else if (K <= 32) k_median_stack<32><<<grid, 256, 0, st>>>(stack, K, n, out);
    else k_median_stack<64><<<grid, 256, 0, st>>>(stack, K, n, out);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_tta_agreement_f64(const double* stack, int K, int64_t nvox, int C, double threshold, double* median, double* mean,
                                      double* variance, double* entropy, double* disagreement, uint64_t* counts, fmri_stream_t stream) {
    if (!stack || !median || K < 1 || K > 64 || C < 1 || C > TTA_MAX_C || nvox <= 0) return FMRI_E_SHAPE;
    const int64_t n = nvox * C;
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(stack), s1 = s0 + (uintptr_t)K * (uintptr_t)n * sizeof(double);
    double* const maps[5] = {median, mean, variance, entropy, disagreement};
    bool wide = C == 1 && nvox % 2 == 0 && K <= 16 && s0 % 16 == 0;
    for (double* m : maps) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(m);
        if (m && a < s1 && a + (uintptr_t)n * sizeof(double) > s0) return FMRI_E_SHAPE;       // an output inside the stack
        wide = wide && a % 16 == 0;
    }
    const size_t count_bytes = (size_t)C * (2 * K + 1) * sizeof(uint64_t);
    const uintptr_t c0 = reinterpret_cast<uintptr_t>(counts);
    if (counts && c0 < s1 && c0 + count_bytes > s0) return FMRI_E_SHAPE;
    hipStream_t st = as_stream(stream);
    if (counts && hipMemsetAsync(counts, 0, count_bytes, st) != hipSuccess) return FMRI_E_LAUNCH;
    const TtaOut o{median, mean, variance, entropy, disagreement};
    unsigned long long* const cnt = reinterpret_cast<unsigned long long*>(counts);
    if (K <= 8) {
        if (wide) tta_go<8, 2>(stack, K, nvox, C, threshold, o, cnt, st);
        else tta_go<8, 1>(stack, K, nvox, C, threshold, o, cnt, st);
    } else if (K <= 16) {
        if (wide) tta_go<16, 2>(stack, K, nvox, C, threshold, o, cnt, st);
        else tta_go<16, 1>(stack, K, nvox, C, threshold, o, cnt, st);
    } else if (K <= 32) {
        tta_go<32, 1>(stack, K, nvox, C, threshold, o, cnt, st);
    } else {
        tta_go<64, 1>(stack, K, nvox, C, threshold, o, cnt, st);
    }
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ---- Fourth: intensity preparation of a whole volume in front of the model (reference prod/predict_nifti2.py:57-74, fetal_net/preprocess.py): the
// percentile window, scipy.ndimage.laplace, the combine step of gaussian_gradient_magnitude and the min-max / z-score maps, all on a
// contiguous fp64 volume.  The antisymmetric 1-D correlation of the gradient is k_correlate1d_sym<., ., true> at the top of the file.
//
// Exactness: every kernel restates numpy's / scipy's own operation order with one rounding per operation (fp contract off; fp64 add,
// multiply, divide and square root are correctly rounded on gfx950 and the Makefile passes no fast-math flag), so the device result is
// the host result bit for bit.  Order statistics are exact by construction: a radix select on the bit patterns.
namespace {

// order-preserving 64-bit key of a double: negatives with all bits flipped, the others with the sign bit flipped.  Every NaN takes the
// largest key (the pattern of a positive NaN with a full mantissa), so NaNs sort last whatever their sign, as np.sort puts them.
constexpr unsigned long long KEY_NAN = ~0ull;
__device__ __forceinline__ unsigned long long f64_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    if (x != x) return KEY_NAN;
    return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
}
__device__ __forceinline__ double key_f64(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? k ^ 0x8000000000000000ull : ~k;
    return __longlong_as_double((long long)b);
}

// ---- order statistics: most-significant-digit radix select of up to 8 ranks at once.
// State in the caller's workspace (all passes are separate launches on one stream: launch order is the only synchronisation):
//   prefix[k]  the key bits of rank k decided so far (low bits zero)      rem[k]  rank k's position among the keys that share its prefix
//   leader[k]  the smallest j with prefix[j] == prefix[k]: ranks that still share a prefix share ONE histogram, row leader[k] - the two
//              ends of a percentile window part only a few digits down, and in the first pass every rank counts every voxel
//   nan        the number of NaNs, counted in the first pass              hist[8][NB] (NB <= 2048) the global histogram of the pass
// A pass = k_select_count (per-workgroup LDS histogram of the digit under the pass, of the keys that match a leader's prefix; its
// non-empty bins are added to hist) then k_select_pick (one workgroup: for each rank the digit whose cumulative count passes rem, new
// prefix / rem / leaders, hist zeroed for the next pass; the last pick writes the values).
constexpr int SEL_MAXK = 8, SEL_MAXNB = 2048;
struct SelState {
    unsigned long long prefix[SEL_MAXK];
    unsigned long long nan;
    unsigned rem[SEL_MAXK];
    int leader[SEL_MAXK];
    unsigned hist[SEL_MAXK * SEL_MAXNB];
};
struct SelRanks {
    unsigned r[SEL_MAXK];
};

__global__ __launch_bounds__(256) void k_select_init(SelState* __restrict__ st, SelRanks ranks, int K) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < SEL_MAXK * SEL_MAXNB; i += gridDim.x * blockDim.x) st->hist[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < SEL_MAXK) {
        const int k = threadIdx.x;
        st->prefix[k] = 0ull;
        st->rem[k] = k < K ? ranks.r[k] : 0u;
        st->leader[k] = 0;                       // nothing decided yet: one histogram serves every rank
        if (k == 0) st->nan = 0ull;
    }
}

// hi = shift + (bits of this digit): keys match a prefix when they agree above bit `hi` (hi == 64: the first pass, every key matches)
template <int NB, int THREADS, bool FIRST>
__global__ __launch_bounds__(THREADS) void k_select_count(const double* __restrict__ src, int64_t n, SelState* __restrict__ st, int K, int shift,
                                                          int hi) {
    __shared__ unsigned h[SEL_MAXK * NB];
    __shared__ unsigned long long s_prefix[SEL_MAXK];
    __shared__ int s_lead[SEL_MAXK];
    if (threadIdx.x < SEL_MAXK) {
        s_prefix[threadIdx.x] = st->prefix[threadIdx.x];
        s_lead[threadIdx.x] = threadIdx.x < K && st->leader[threadIdx.x] == (int)threadIdx.x ? 1 : 0;
    }
    __syncthreads();
    for (int k = 0; k < K; ++k)
        if (s_lead[k])
            for (int b = threadIdx.x; b < NB; b += THREADS) h[k * NB + b] = 0u;
    __syncthreads();
    unsigned nans = 0;
    const unsigned mask = (1u << (hi - shift)) - 1u;         // hi - shift <= log2(NB) bits in this digit
    for (int64_t t = (int64_t)blockIdx.x * THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * THREADS) {
        const unsigned long long key = f64_key(src[t]);
        if (FIRST) nans += key == KEY_NAN ? 1u : 0u;
        const unsigned digit = (unsigned)(key >> shift) & mask;
        for (int k = 0; k < K; ++k)
            if (s_lead[k] && (FIRST || (key >> hi) == (s_prefix[k] >> hi))) atomicAdd(&h[k * NB + digit], 1u);
    }
    __syncthreads();
    for (int k = 0; k < K; ++k)
        if (s_lead[k])
            for (int b = threadIdx.x; b < NB; b += THREADS) {
                const unsigned c = h[k * NB + b];
                if (c) atomicAdd(&st->hist[k * SEL_MAXNB + b], c);
            }
    if (FIRST) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) nans += __shfl_xor(nans, o);
        if ((threadIdx.x & 63) == 0 && nans) atomicAdd(&st->nan, (unsigned long long)nans);
    }
}

template <int NB>
__global__ __launch_bounds__(256) void k_select_pick(SelState* __restrict__ st, int K, int shift, int last, double* __restrict__ out,
                                                     long long* __restrict__ nan_count) {
    constexpr int E = NB / 256;                  // bins per thread, contiguous
    __shared__ unsigned scan[256];
    __shared__ unsigned long long s_prefix[SEL_MAXK];
    __shared__ unsigned s_rem[SEL_MAXK];
    const int tid = threadIdx.x;
    for (int lead = 0; lead < K; ++lead) {
        if (st->leader[lead] != lead) continue;  // uniform: read from global by every thread
        unsigned c[E], sum = 0;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            c[e] = st->hist[lead * SEL_MAXNB + tid * E + e];
            sum += c[e];
        }
        scan[tid] = sum;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {      // inclusive scan of the per-thread sums
            const unsigned v = tid >= o ? scan[tid - o] : 0u;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const unsigned base = scan[tid] - sum;   // keys in the bins below this thread's
        for (int k = lead; k < K; ++k) {
            if (st->leader[k] != lead) continue;
            const unsigned want = st->rem[k];
            unsigned below = base;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                if (c[e] && want >= below && want - below < c[e]) {      // exactly one bin of one thread
                    s_prefix[k] = st->prefix[k] | ((unsigned long long)(tid * E + e) << shift);
                    s_rem[k] = want - below;
                }
                below += c[e];
            }
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < E; ++e) st->hist[lead * SEL_MAXNB + tid * E + e] = 0u;
    }
    __syncthreads();
    if (tid < K) {
        st->prefix[tid] = s_prefix[tid];
        st->rem[tid] = s_rem[tid];
        int lead = tid;
        for (int j = tid - 1; j >= 0; --j)
            if (s_prefix[j] == s_prefix[tid]) lead = j;
        st->leader[tid] = lead;
        if (last) out[tid] = key_f64(s_prefix[tid]);
    }
    if (last && tid == 0) *nan_count = (long long)st->nan;
}

template <int BITS>
int select_run(const double* src, int64_t n, SelState* st, const SelRanks& ranks, int K, double* out, long long* nan_count, hipStream_t s) {
    constexpr int NB = 1 << BITS, THREADS = BITS > 8 ? 1024 : 256;
    k_select_init<<<16, 256, 0, s>>>(st, ranks, K);
    const int grid = grid_for(n, THREADS, 256);              // one flush of up to K * NB atomics per workgroup and pass: one per CU
    for (int hi = 64; hi > 0; hi -= BITS) {
        const int shift = hi > BITS ? hi - BITS : 0;         // the last digit of the 11-bit form has 9 bits
        if (hi == 64) k_select_count<NB, THREADS, true><<<grid, THREADS, 0, s>>>(src, n, st, K, shift, hi);
        else k_select_count<NB, THREADS, false><<<grid, THREADS, 0, s>>>(src, n, st, K, shift, hi);
        k_select_pick<NB><<<1, 256, 0, s>>>(st, K, shift, shift == 0 ? 1 : 0, out, nan_count);
    }
    return hipGetLastError() == hipSuccess ? FMRI_OK : FMRI_E_LAUNCH;
}

// ---- range of a volume: min / max through integer atomics on the ordered keys (fmin / fmax skip NaNs; they are counted instead)
__global__ void k_minmax64_init(unsigned long long* mm, long long* nan_count) {
    mm[0] = ~0ull;
    mm[1] = 0ull;
    *nan_count = 0;
}
__global__ __launch_bounds__(256) void k_minmax64(const double* __restrict__ x, int64_t n, unsigned long long* mm, long long* nan_count) {
    unsigned long long lo = ~0ull, hi = 0ull;
    unsigned nans = 0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const double v = x[t];
        if (v != v) {
            ++nans;
        } else {
            const unsigned long long k = f64_key(v);
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long l2 = __shfl_xor(lo, o), h2 = __shfl_xor(hi, o);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
        nans += __shfl_xor(nans, o);
    }
    if ((threadIdx.x & 63) == 0) {
        if (lo <= hi) {
            atomicMin(&mm[0], lo);
            atomicMax(&mm[1], hi);
        }
        if (nans) atomicAdd((unsigned long long*)nan_count, (unsigned long long)nans);
    }
}
__global__ void k_minmax64_decode(unsigned long long* mm) {
    const double lo = key_f64(mm[0]), hi = key_f64(mm[1]);      // no finite value at all: the initial keys decode to NaNs
    reinterpret_cast<double*>(mm)[0] = lo;
    reinterpret_cast<double*>(mm)[1] = hi;
}

// ---- element-wise maps, each in the host expression's own operation order
//   FMRI_MAP_WINDOW   (min(max(x, lo), hi) - lo) * scale + out_min      np.clip's min / max: a NaN x stays, a NaN bound wins
//   FMRI_MAP_MINMAX   -1 + (2 * (x - mn)) / (mx - mn)
//   FMRI_MAP_ZSCORE   (x - mean) / std
template <int KIND>
__global__ __launch_bounds__(256) void k_intensity_map(const double* src, double* dst, int64_t n, double p0, double p1, double p2, double p3) {
#pragma clang fp contract(off)
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const double x = src[t];
        double y;
        if (KIND == FMRI_MAP_WINDOW) {
            const double a = x != x ? x : (x > p0 ? x : p0);
            const double b = a != a ? a : (a < p1 ? a : p1);
            y = (b - p0) * p2 + p3;
        } else if (KIND == FMRI_MAP_MINMAX) {
            y = -1.0 + (2.0 * (x - p0)) / (p1 - p0);
        } else {
            y = (x - p0) / p1;
        }
        dst[t] = y;
    }
}

// scipy.ndimage.laplace, mode 'reflect': per axis correlate1d with [1, -2, 1] (NI_Correlate1D's symmetric branch, centre tap first), the
// axes' results added in ascending order.  One thread per voxel, z fastest; the six neighbours come from cache.
__global__ __launch_bounds__(256) void k_laplace(const double* __restrict__ src, double* __restrict__ dst, int X, int Y, int Z) {
#pragma clang fp contract(off)
    const int64_t total = (int64_t)X * Y * Z, sx = (int64_t)Y * Z;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int z = (int)(t % Z);
        const int64_t q = t / Z;
        const int y = (int)(q % Y), x = (int)(q / Y);
        const double c = src[t];
        const double l0 = c * -2.0 + (src[t + (int64_t)(reflect_idx(x - 1, X) - x) * sx] + src[t + (int64_t)(reflect_idx(x + 1, X) - x) * sx]) * 1.0;
        const double l1 = c * -2.0 + (src[t + (int64_t)(reflect_idx(y - 1, Y) - y) * Z] + src[t + (int64_t)(reflect_idx(y + 1, Y) - y) * Z]) * 1.0;
        const double l2 = c * -2.0 + (src[t + (reflect_idx(z - 1, Z) - z)] + src[t + (reflect_idx(z + 1, Z) - z)]) * 1.0;
        dst[t] = (l0 + l1) + l2;
    }
}

// the tail of scipy.ndimage.generic_gradient_magnitude: squares added in axis order, then the square root
__global__ __launch_bounds__(256) void k_grad_combine(const double* d0, const double* d1, const double* d2, double* out, int64_t n) {
#pragma clang fp contract(off)
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += (int64_t)gridDim.x * blockDim.x) {
        const double a = d0[t], b = d1[t], c = d2[t];
        out[t] = sqrt((a * a + b * b) + c * c);
    }
}

// ---- moments of a volume: what numpy's ndarray.mean() / ndarray.std() compute (sum / n; a SECOND pass for sqrt(sum((x - mean)^2) / n)),
// with min, max and the NaN count of k_minmax64 taken in the first pass.  Two launches per pass: k_moments_partials leaves one partial
// per workgroup in the workspace, k_moments_finish (one workgroup) combines them in index order.  Every sum is a pair {s, c} in
// Neumaier's form (s the running sum, c the rounding errors it dropped; the value is s + c) from the lane's own loop up to the last
// combine, so the result is within a few ulp of the exact sum whatever n is; where every partial sum is exactly representable (integer
// volumes) c stays 0 and the sum is exact.  Order: a lane adds the element pairs 2p, 2p + 1 for p = its index, + lanes, + 2 * lanes ...;
// lanes combine in a fixed tree (wave by shuffles, the four waves through LDS, the workgroups in k_moments_finish).  The grid is a
// function of n alone and the pair a lane reads does not depend on how it is loaded (one 16-byte load, or two 8-byte loads for a src that
// is not 16-byte aligned), so the same values give the same bits on every run, device and alignment.
constexpr int MOM_THREADS = 256, MOM_WAVES = MOM_THREADS / 64, MOM_GRID = 2048, MOM_PAIRS = 8;     // pairs per lane before the grid saturates
struct MomPartial {
    double s, c;
    unsigned long long lo, hi, nans;
};
// (MomSum, mom_add and mom_merge - the compensated pair and its two steps - are in common.h: fmri_grad_sumsq sums the same way)

template <bool VEC, int PASS>       // PASS 0: sum, min / max keys, NaN count of x;  PASS 1: sum of (x - *mean)^2
__global__ __launch_bounds__(MOM_THREADS) void k_moments_partials(const double* __restrict__ x, int64_t n, const double* __restrict__ mean,
                                                                 MomPartial* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ MomPartial part[MOM_WAVES];
    const double m = PASS ? *mean : 0.0;
    MomSum acc{0.0, 0.0};
    unsigned long long lo = ~0ull, hi = 0ull, nans = 0;
    auto take = [&](double v) {
        if (PASS) {
            const double d = v - m;
            mom_add(acc, d * d);
        } else {
            mom_add(acc, v);
            if (v != v) {
                ++nans;
            } else {
                const unsigned long long k = f64_key(v);
                lo = k < lo ? k : lo;
                hi = k > hi ? k : hi;
            }
        }
    };
    const int64_t pairs = n >> 1, step = (int64_t)gridDim.x * MOM_THREADS;
    for (int64_t p = (int64_t)blockIdx.x * MOM_THREADS + threadIdx.x; p < pairs; p += step) {
        double a, b;
        if (VEC) {
            const double2 v = *reinterpret_cast<const double2*>(x + 2 * p);
            a = v.x;
            b = v.y;
        } else {
            a = x[2 * p];
            b = x[2 * p + 1];
        }
        take(a);
        take(b);
    }
    if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) take(x[n - 1]);       // the odd last element
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                                        // lane 0 ends with the wave's tree
        const double bs = __shfl_down(acc.s, o), bc = __shfl_down(acc.c, o);
        mom_merge(acc, bs, bc);
        if (!PASS) {
            const unsigned long long l2 = __shfl_down(lo, o), h2 = __shfl_down(hi, o);
            lo = l2 < lo ? l2 : lo;
            hi = h2 > hi ? h2 : hi;
            nans += __shfl_down(nans, o);
        }
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = MomPartial{acc.s, acc.c, lo, hi, nans};
    __syncthreads();
    if (threadIdx.x == 0) {
        MomPartial r = part[0];
        MomSum t{r.s, r.c};
        for (int w = 1; w < MOM_WAVES; ++w) {
            mom_merge(t, part[w].s, part[w].c);
            r.lo = part[w].lo < r.lo ? part[w].lo : r.lo;
            r.hi = part[w].hi > r.hi ? part[w].hi : r.hi;
            r.nans += part[w].nans;
        }
        r.s = t.s;
        r.c = t.c;
        partial[blockIdx.x] = r;
    }
}

// one workgroup: thread i combines partials i, i + 256, ... in that order, then a fixed tree over the 256 threads.  PASS 0 writes
// out5[0] = mean, [2] = min, [3] = max, [4] = sum and *nan_count; PASS 1 writes out5[1] = std.
template <int PASS>
__global__ __launch_bounds__(MOM_THREADS) void k_moments_finish(const MomPartial* __restrict__ partial, int parts, int64_t n, double* __restrict__ out5,
                                                               long long* __restrict__ nan_count) {
#pragma clang fp contract(off)
    __shared__ MomPartial sh[MOM_THREADS];
    MomSum acc{0.0, 0.0};
    unsigned long long lo = ~0ull, hi = 0ull, nans = 0;
    for (int i = threadIdx.x; i < parts; i += MOM_THREADS) {
        const MomPartial p = partial[i];
        mom_merge(acc, p.s, p.c);
        lo = p.lo < lo ? p.lo : lo;
        hi = p.hi > hi ? p.hi : hi;
        nans += p.nans;
    }
    sh[threadIdx.x] = MomPartial{acc.s, acc.c, lo, hi, nans};
    __syncthreads();
    for (int o = MOM_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            MomPartial a = sh[threadIdx.x];
            const MomPartial b = sh[threadIdx.x + o];
            MomSum t{a.s, a.c};
            mom_merge(t, b.s, b.c);
            a.s = t.s;
            a.c = t.c;
            a.lo = b.lo < a.lo ? b.lo : a.lo;
            a.hi = b.hi > a.hi ? b.hi : a.hi;
            a.nans += b.nans;
            sh[threadIdx.x] = a;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double total = sh[0].s + sh[0].c;
        if (PASS) {
            out5[1] = sqrt(total / (double)n);
        } else {
            out5[0] = total / (double)n;
            out5[2] = key_f64(sh[0].lo);               // no value that is not a NaN: the initial keys decode to NaNs, as in k_minmax64_decode
            out5[3] = key_f64(sh[0].hi);
            out5[4] = total;
            *nan_count = (long long)sh[0].nans;
        }
    }
}

}  // namespace

extern "C" int64_t fmri_order_stats_workspace_bytes(void) { return (int64_t)sizeof(SelState); }

extern "C" int fmri_order_stats_f64(const double* src, int64_t n, const int64_t* ranks_host, int K, double* out, int64_t* nan_count,
                                    void* workspace, fmri_stream_t stream) {
    if (!src || !ranks_host || !out || !nan_count || !workspace || n <= 0 || n >= ((int64_t)1 << 31) || K < 1 || K > SEL_MAXK)
        return FMRI_E_SHAPE;
    SelRanks ranks{};
    for (int k = 0; k < K; ++k) {
        if (ranks_host[k] < 0 || ranks_host[k] >= n) return FMRI_E_SHAPE;
        ranks.r[k] = (unsigned)ranks_host[k];
    }
    // digit width: 6 passes of 11 bits, or 8 passes of 8 bits.  Measured on a 160x256x256 volume (tools/bench_intensity.py, which is why
    // the switch is read per call: one process times both): 4 ranks in 0.31-0.39 ms with 11 bits, 1.0-1.07 ms with 8.
    const int bits = env_int("FMRI_SELECT_BITS", 11, {8, 11});
    SelState* st = static_cast<SelState*>(workspace);
    long long* nc = reinterpret_cast<long long*>(nan_count);
    return bits == 11 ? select_run<11>(src, n, st, ranks, K, out, nc, as_stream(stream))
                      : select_run<8>(src, n, st, ranks, K, out, nc, as_stream(stream));
}

extern "C" int fmri_minmax_f64(const double* src, int64_t n, double* out2, int64_t* nan_count, fmri_stream_t stream) {
    if (!src || !out2 || !nan_count || n <= 0) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    unsigned long long* mm = reinterpret_cast<unsigned long long*>(out2);
    long long* nc = reinterpret_cast<long long*>(nan_count);
    k_minmax64_init<<<1, 1, 0, s>>>(mm, nc);
    k_minmax64<<<grid_for(n, 256, 2048), 256, 0, s>>>(src, n, mm, nc);
    k_minmax64_decode<<<1, 1, 0, s>>>(mm);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int64_t fmri_moments_workspace_bytes(void) { return (int64_t)(MOM_GRID * sizeof(MomPartial)); }

extern "C" int fmri_moments_f64(const double* src, int64_t n, double* out5, int64_t* nan_count, void* workspace, fmri_stream_t stream) {
    if (!src || !out5 || !nan_count || !workspace || n <= 0 || (reinterpret_cast<uintptr_t>(src) & 7u)) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    MomPartial* const partial = static_cast<MomPartial*>(workspace);
    long long* const nc = reinterpret_cast<long long*>(nan_count);
    const int parts = grid_for(ceil_div64(n >> 1, MOM_PAIRS), MOM_THREADS, MOM_GRID);       // a function of n alone
    if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
        k_moments_partials<true, 0><<<parts, MOM_THREADS, 0, s>>>(src, n, nullptr, partial);
        k_moments_finish<0><<<1, MOM_THREADS, 0, s>>>(partial, parts, n, out5, nc);
        k_moments_partials<true, 1><<<parts, MOM_THREADS, 0, s>>>(src, n, out5, partial);
    } else {
        k_moments_partials<false, 0><<<parts, MOM_THREADS, 0, s>>>(src, n, nullptr, partial);
        k_moments_finish<0><<<1, MOM_THREADS, 0, s>>>(partial, parts, n, out5, nc);
        k_moments_partials<false, 1><<<parts, MOM_THREADS, 0, s>>>(src, n, out5, partial);
    }
    k_moments_finish<1><<<1, MOM_THREADS, 0, s>>>(partial, parts, n, out5, nc);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_intensity_map_f64(const double* src, double* dst, int64_t n, int kind, double p0, double p1, double p2, double p3,
                                      fmri_stream_t stream) {
    if (!src || !dst || n <= 0 || kind < FMRI_MAP_WINDOW || kind > FMRI_MAP_ZSCORE) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    const int grid = grid_for(n, 256, 8192);
    if (kind == FMRI_MAP_WINDOW) k_intensity_map<FMRI_MAP_WINDOW><<<grid, 256, 0, s>>>(src, dst, n, p0, p1, p2, p3);
    else if (kind == FMRI_MAP_MINMAX) k_intensity_map<FMRI_MAP_MINMAX><<<grid, 256, 0, s>>>(src, dst, n, p0, p1, p2, p3);
    else k_intensity_map<FMRI_MAP_ZSCORE><<<grid, 256, 0, s>>>(src, dst, n, p0, p1, p2, p3);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_laplace_f64(const double* src, double* dst, int X, int Y, int Z, fmri_stream_t stream) {
    if (!src || !dst || src == dst || X <= 0 || Y <= 0 || Z <= 0) return FMRI_E_SHAPE;
    k_laplace<<<grid_for((int64_t)X * Y * Z, 256, 8192), 256, 0, as_stream(stream)>>>(src, dst, X, Y, Z);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_grad_magnitude_combine_f64(const double* d0, const double* d1, const double* d2, double* out, int64_t n,
                                               fmri_stream_t stream) {
    if (!d0 || !d1 || !d2 || !out || n <= 0) return FMRI_E_SHAPE;
    k_grad_combine<<<grid_for(n, 256, 8192), 256, 0, as_stream(stream)>>>(d0, d1, d2, out, n);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ---- Fifth: scoring a predicted mask against the truth (reference fetal/evaluate.py: hard Dice on "> 0" masks; the surface metrics are
// medpy.metric.binary's hd / hd95 / assd restated).  Two uint8 volumes [X][Y][Z], a voxel belongs to a mask when its byte is nonzero.
//   counts     |A|, |B|, |A n B|: the overlap scores (Dice, VOD, volume difference, sensitivity, precision) are ratios of these integers.
//   surface    border = mask ^ binary_erosion(mask, generate_binary_structure(3, connectivity)), scipy's border_value = 0: a foreground
//              voxel with a background neighbour, or with a neighbour outside the volume.  Written INVERTED (0 on the border, 1 elsewhere):
//              that is the input of fmri_edt_u8, whose field is then the distance of every voxel to the nearest border voxel -
//              distance_transform_edt(~border, sampling).
//   distances  d(A -> B) = that field of B read at A's border voxels.  Its sum and maximum come from one masked reduction, the percentile
//              from a stream compaction of both directions into one buffer followed by the radix select above.
// Exactness: counts, borders and maxima are exact; the distances are the EDT's (identical to scipy at unit spacing).  The sum is
// reproducible: the grid depends on n alone, every thread adds its voxels in index order, a wave adds by a fixed butterfly, the waves of a
// workgroup and then the workgroups' partials are added in index order by a second launch.  No floating-point atomics anywhere.
namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_GRID = 2048;            // cap of the voxel kernels' grids (8 workgroups per CU); also the number of partials
constexpr int EV_WAVES = EV_THREADS / 64;

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// bit 7 of every nonzero byte of w
__device__ __forceinline__ unsigned long long nonzero_bytes(unsigned long long w) {
    return (((w & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | w) & 0x8080808080808080ull;
}

// words = n / 8 when both pointers are 8-byte aligned (eight voxels per load), else 0; the remaining voxels go one per thread
__global__ __launch_bounds__(EV_THREADS) void k_seg_counts(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, int64_t n, int64_t words,
                                                           unsigned long long* __restrict__ out) {
    __shared__ unsigned long long part[3][EV_WAVES];
    unsigned long long ca = 0, cb = 0, cab = 0;
    const int64_t tid = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x, step = (int64_t)gridDim.x * EV_THREADS;
    const unsigned long long* const a8 = reinterpret_cast<const unsigned long long*>(a);
    const unsigned long long* const b8 = reinterpret_cast<const unsigned long long*>(b);
    for (int64_t t = tid; t < words; t += step) {
        const unsigned long long ma = nonzero_bytes(a8[t]), mb = nonzero_bytes(b8[t]);
        ca += __popcll(ma);
        cb += __popcll(mb);
        cab += __popcll(ma & mb);
    }
    for (int64_t t = words * 8 + tid; t < n; t += step) {
        const int va = a[t] != 0, vb = b[t] != 0;
        ca += va;
        cb += vb;
        cab += va & vb;
    }
    ca = wave_sum_u64(ca);
    cb = wave_sum_u64(cb);
    cab = wave_sum_u64(cab);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        part[0][wave] = ca;
        part[1][wave] = cb;
        part[2][wave] = cab;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        unsigned long long s = 0;
        for (int w = 0; w < EV_WAVES; ++w) s += part[threadIdx.x][w];
        if (s) atomicAdd(&out[threadIdx.x], s);
    }
}

// out[l] = {|T == v_l|, |P == v_l|, |both|} for all labels in one pass.  The bytes go through a 256-entry value -> index table in LDS; a wave
// counts by vote, not by lane: the lanes whose (truth index, prediction index) pair equals the first unsettled lane's are counted with one
// ballot and their number is added to the workgroup's LDS counters by that lane - label regions are contiguous, so a wave holds a few
// distinct pairs and most waves none (all background: one ballot).  The workgroup's counters then go out as 64-bit integer atomics.
// words = n / 4 when both pointers are 4-byte aligned (four voxels per load), else 0; the remaining voxels go one per thread.
__device__ __forceinline__ void label_vote(int it, int ip, unsigned* __restrict__ cnt) {
    const int key = it * (FMRI_MAX_LABELS + 1) + ip;
    unsigned long long todo = __ballot(key != 0);
    const int lane = threadIdx.x & 63;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader);
        const unsigned long long same = __ballot(key == k) & todo;
        if (lane == leader) {
            const unsigned c = (unsigned)__popcll(same);
            if (it) atomicAdd(&cnt[3 * (it - 1)], c);
            if (ip) atomicAdd(&cnt[3 * (ip - 1) + 1], c);
            if (it && it == ip) atomicAdd(&cnt[3 * (it - 1) + 2], c);
        }
        todo &= ~same;
    }
}
__global__ __launch_bounds__(EV_THREADS) void k_label_counts(const uint8_t* __restrict__ truth, const uint8_t* __restrict__ pred, int64_t n,
                                                             int64_t words, int L, unsigned long long* __restrict__ out, FmriLabelValues V) {
    __shared__ __attribute__((aligned(4))) uint8_t vals[FMRI_MAX_LABELS];
    __shared__ uint8_t lut[256];
    __shared__ unsigned cnt[3 * FMRI_MAX_LABELS];
    if (threadIdx.x < 3 * FMRI_MAX_LABELS) cnt[threadIdx.x] = 0;
    fmri_label_tables(V, L, vals, lut);
    // every lane of a wave makes the same number of trips (the votes need the whole wave): the loops run on the wave's first index
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * EV_THREADS + (threadIdx.x - lane), step = (int64_t)gridDim.x * EV_THREADS;
    const uint32_t* const t4 = reinterpret_cast<const uint32_t*>(truth);
    const uint32_t* const p4 = reinterpret_cast<const uint32_t*>(pred);
    for (int64_t w0 = wave0; w0 < words; w0 += step) {
        const int64_t w = w0 + lane;
        const uint32_t a = w < words ? t4[w] : 0u, b = w < words ? p4[w] : 0u;
        if (__ballot((a | b) != 0) == 0) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) label_vote(lut[(a >> (8 * j)) & 255u], lut[(b >> (8 * j)) & 255u], cnt);
    }
    for (int64_t v0 = words * 4 + wave0; v0 < n; v0 += step) {
        const int64_t v = v0 + lane;
        label_vote(v < n ? lut[truth[v]] : 0, v < n ? lut[pred[v]] : 0, cnt);
    }
    __syncthreads();
    if (threadIdx.x < 3 * L && cnt[threadIdx.x]) atomicAdd(&out[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

// blockIdx.y selects the volume (one or two in a launch).  CONN = scipy's connectivity: the neighbours with 1 .. CONN nonzero offsets.
template <int CONN>
__global__ __launch_bounds__(EV_THREADS) void k_surface(const uint8_t* __restrict__ m0, const uint8_t* __restrict__ m1, uint8_t* __restrict__ i0,
                                                        uint8_t* __restrict__ i1, int X, int Y, int Z, unsigned long long* __restrict__ count) {
    __shared__ unsigned long long part[EV_WAVES];
    const uint8_t* const __restrict__ mask = blockIdx.y ? m1 : m0;
    uint8_t* const __restrict__ inv = blockIdx.y ? i1 : i0;
    const int64_t total = (int64_t)X * Y * Z, sx = (int64_t)Y * Z;
    unsigned long long found = 0;
    for (int64_t t = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x; t < total; t += (int64_t)gridDim.x * EV_THREADS) {
        int border = 0;
        if (mask[t]) {
            const int z = (int)(t % Z);
            const int64_t q = t / Z;
            const int y = (int)(q % Y), x = (int)(q / Y);
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx)
#pragma unroll
                for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                    for (int dz = -1; dz <= 1; ++dz) {
                        const int order = (dx != 0) + (dy != 0) + (dz != 0);
                        if (order == 0 || order > CONN) continue;
                        const int xx = x + dx, yy = y + dy, zz = z + dz;
                        if (xx < 0 || xx >= X || yy < 0 || yy >= Y || zz < 0 || zz >= Z) border = 1;
                        else if (!mask[t + dx * sx + dy * (int64_t)Z + dz]) border = 1;
                    }
        }
        inv[t] = border ? 0 : 1;
        found += border;
    }
    found = wave_sum_u64(found);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = found;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int w = 0; w < EV_WAVES; ++w) s += part[w];
        if (s) atomicAdd(&count[blockIdx.y], s);
    }
}

// partial[2 * blockIdx.x] = {sum, max} of the workgroup's selected values; the grid is a function of n alone (see above)
__global__ __launch_bounds__(EV_THREADS) void k_masked_partials(const double* __restrict__ values, const uint8_t* __restrict__ inv_sel, int64_t n,
                                                                double* __restrict__ partial) {
    __shared__ double ps[EV_WAVES], pm[EV_WAVES];
    double sum = 0.0, mx = -(double)INFINITY;
    for (int64_t t = (int64_t)blockIdx.x * EV_THREADS + threadIdx.x; t < n; t += (int64_t)gridDim.x * EV_THREADS)
        if (inv_sel[t] == 0) {
            const double v = values[t];
            sum += v;
            mx = fmax(mx, v);
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o);
        mx = fmax(mx, __shfl_xor(mx, o));
    }
    if ((threadIdx.x & 63) == 0) {
        ps[threadIdx.x >> 6] = sum;
        pm[threadIdx.x >> 6] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = ps[0], m = pm[0];
        for (int w = 1; w < EV_WAVES; ++w) {
            s += ps[w];
            m = fmax(m, pm[w]);
        }
        partial[2 * blockIdx.x] = s;
        partial[2 * blockIdx.x + 1] = m;
    }
}

// one workgroup: thread i adds partials i, i + 256, ... in that order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(EV_THREADS) void k_masked_finish(const double* __restrict__ partial, int parts, double* __restrict__ out) {
    __shared__ double ss[EV_THREADS], sm[EV_THREADS];
    double sum = 0.0, mx = -(double)INFINITY;
    for (int i = threadIdx.x; i < parts; i += EV_THREADS) {
        sum += partial[2 * i];
        mx = fmax(mx, partial[2 * i + 1]);
    }
    ss[threadIdx.x] = sum;
    sm[threadIdx.x] = mx;
    __syncthreads();
    for (int o = EV_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            ss[threadIdx.x] += ss[threadIdx.x + o];
            sm[threadIdx.x] = fmax(sm[threadIdx.x], sm[threadIdx.x + o]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = ss[0];
        out[1] = sm[0];
    }
}

// the selected values, dense, from out[*cursor] on.  Every wave owns one contiguous run of voxels (a multiple of 64, so its loads of
// inv_sel are whole 64-byte lines) and walks it twice: first it counts its selected voxels by ballots; thread 0 then reserves the
// workgroup's total with ONE integer atomic and hands every wave its start; the second walk (inv_sel now comes from cache) ballots
// again and every selected lane stores at the wave's running start + the number of selected lanes below it.  One atomic per wave and
// ballot, the first form of this kernel, put ~40 k atomics on the one cursor: 0.22 ms for a 160x256x256 volume, 15x the masked
// reduction that reads the same bytes.  The loop bounds are uniform over a wave, so all 64 lanes reach every ballot.  A slot at or past
// `capacity` is not written (the cursor still advances: the caller compares).
__global__ __launch_bounds__(EV_THREADS) void k_masked_compact(const double* __restrict__ values, const uint8_t* __restrict__ inv_sel, int64_t n,
                                                               double* __restrict__ out, int64_t capacity, unsigned long long* __restrict__ cursor) {
    __shared__ unsigned long long wcount[EV_WAVES], wstart[EV_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t waves = (int64_t)gridDim.x * EV_WAVES;
    const int64_t per = ((n + waves - 1) / waves + 63) / 64 * 64;
    const int64_t w = (int64_t)blockIdx.x * EV_WAVES + wave;
    const int64_t lo = min(w * per, n), hi = min(lo + per, n);
    unsigned long long count = 0;
    for (int64_t t0 = lo; t0 < hi; t0 += 64) {
        const int64_t t = t0 + lane;
        count += __popcll(__ballot(t < hi && inv_sel[t] == 0));
    }
    if (lane == 0) wcount[wave] = count;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long total = 0;
        for (int k = 0; k < EV_WAVES; ++k) total += wcount[k];
        unsigned long long at = total ? atomicAdd(cursor, total) : 0ull;
        for (int k = 0; k < EV_WAVES; ++k) {
            wstart[k] = at;
            at += wcount[k];
        }
    }
    __syncthreads();
    unsigned long long at = wstart[wave];
    for (int64_t t0 = lo; t0 < hi; t0 += 64) {
        const int64_t t = t0 + lane;
        const bool sel = t < hi && inv_sel[t] == 0;
        const unsigned long long vote = __ballot(sel);
        if (sel) {
            const int64_t slot = (int64_t)at + __popcll(vote & ((1ull << lane) - 1ull));
            if (slot < capacity) out[slot] = values[t];
        }
        at += __popcll(vote);
    }
}

}  // namespace

extern "C" int fmri_seg_counts_u8(const uint8_t* a, const uint8_t* b, int64_t n, int64_t* out3, fmri_stream_t stream) {
    if (!a || !b || !out3 || n <= 0) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(out3, 0, 3 * sizeof(int64_t), s) != hipSuccess) return FMRI_E_LAUNCH;
    const bool aligned = ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7u) == 0;
    const int64_t words = aligned ? n / 8 : 0;
    k_seg_counts<<<grid_for(aligned ? words : n, EV_THREADS, EV_GRID), EV_THREADS, 0, s>>>(a, b, n, words,
                                                                                                  reinterpret_cast<unsigned long long*>(out3));
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_label_counts_u8(const uint8_t* truth, const uint8_t* pred, int64_t n, const uint8_t* values, int L, int64_t* out,
                                    fmri_stream_t stream) {
    FmriLabelValues V;
    if (!truth || !pred || !out || n <= 0 || fmri_label_values(values, L, &V) != FMRI_OK) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(out, 0, (size_t)3 * L * sizeof(int64_t), s) != hipSuccess) return FMRI_E_LAUNCH;
    const bool aligned = ((reinterpret_cast<uintptr_t>(truth) | reinterpret_cast<uintptr_t>(pred)) & 3u) == 0;
    const int64_t words = aligned ? n / 4 : 0;
    k_label_counts<<<grid_for(aligned ? words + 3 : n, EV_THREADS, EV_GRID), EV_THREADS, 0, s>>>(truth, pred, n, words, L,
                                                                                                   reinterpret_cast<unsigned long long*>(out), V);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_surface_u8(const uint8_t* mask, uint8_t* inv_border, const uint8_t* mask2, uint8_t* inv_border2, int X, int Y, int Z,
                               int connectivity, int64_t* count, fmri_stream_t stream) {
    if (!mask || !inv_border || mask == inv_border || !count || X <= 0 || Y <= 0 || Z <= 0 || connectivity < 1 || connectivity > 3)
        return FMRI_E_SHAPE;
    const int nvol = mask2 ? 2 : 1;
    if (mask2 && (!inv_border2 || mask2 == inv_border2 || inv_border2 == inv_border || inv_border2 == mask || inv_border == mask2))
        return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(count, 0, nvol * sizeof(int64_t), s) != hipSuccess) return FMRI_E_LAUNCH;
    const dim3 grid(grid_for((int64_t)X * Y * Z, EV_THREADS, EV_GRID), nvol);
    unsigned long long* const c = reinterpret_cast<unsigned long long*>(count);
    if (connectivity == 1) k_surface<1><<<grid, EV_THREADS, 0, s>>>(mask, mask2, inv_border, inv_border2, X, Y, Z, c);
    else if (connectivity == 2) k_surface<2><<<grid, EV_THREADS, 0, s>>>(mask, mask2, inv_border, inv_border2, X, Y, Z, c);
    else k_surface<3><<<grid, EV_THREADS, 0, s>>>(mask, mask2, inv_border, inv_border2, X, Y, Z, c);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int64_t fmri_masked_stats_workspace_bytes(void) { return (int64_t)(2 * EV_GRID * sizeof(double)); }

extern "C" int fmri_masked_stats_f64(const double* values, const uint8_t* inv_sel, int64_t n, double* out2, void* workspace,
                                     fmri_stream_t stream) {
    if (!values || !inv_sel || !out2 || !workspace || n <= 0) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    const int parts = grid_for(n, EV_THREADS, EV_GRID);
    double* const partial = static_cast<double*>(workspace);
    k_masked_partials<<<parts, EV_THREADS, 0, s>>>(values, inv_sel, n, partial);
    k_masked_finish<<<1, EV_THREADS, 0, s>>>(partial, parts, out2);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_masked_compact_f64(const double* values, const uint8_t* inv_sel, int64_t n, double* out, int64_t capacity, int64_t* cursor,
                                       fmri_stream_t stream) {
    if (!values || !inv_sel || !out || !cursor || n <= 0 || capacity <= 0) return FMRI_E_SHAPE;
    k_masked_compact<<<grid_for(n, EV_THREADS, EV_GRID), EV_THREADS, 0, as_stream(stream)>>>(values, inv_sel, n, out, capacity,
                                                                                             reinterpret_cast<unsigned long long*>(cursor));
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
