// HBM-bound kernels of the U-Net step: pooling, up-sampling, final 1x1x1 conv, sigmoid+Dice, Adam, weight packing,
// sliding-window tile gather / overlap-add, casts.  All channels-last, vectorised where the channel count allows.
#include <cstdlib>
#include <type_traits>
#include "common.h"

FMRI_DET_TU(pointwise)
static __device__ unsigned long long g_isums[16];      // metric sums of the deterministic mode, 2^-20 fixed point

// ------------------------------------------------------------------------------------------------ version / errors
extern "C" int fmri_version(void) { return 100; }
extern "C" const char* fmri_error_string(int code) {
    switch (code) {
        case FMRI_OK: return "ok";
        case FMRI_E_SHAPE: return "unsupported shape";
        case FMRI_E_ALIGN: return "misaligned pointer";
        case FMRI_E_ARCH: return "unsupported architecture";
        case FMRI_E_LAUNCH: return "kernel launch failed";
        case FMRI_E_DTYPE: return "unsupported dtype";
        default: return "unknown error";
    }
}

// ------------------------------------------------------------------------------------------------ shader-clock stamps (measurement aid)
// One (s_memtime, s_memrealtime) pair per XCD: s_memtime ticks with the shader clock, s_memrealtime at a constant 100 MHz, so two stamps
// bracket a region's average shader clock: d(memtime) / d(memrealtime) x 0.1 GHz (MI355X guide, 'DVFS give-back' item 6).  The counters
// are per XCD, so a workgroup writes the slot of the XCD it runs on (HW_REG_XCC_ID); 64 workgroups reach all eight.
__global__ void k_clock_stamp(unsigned long long* out) {
    if (threadIdx.x != 0) return;
    const unsigned xcc = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20) & 7u;       // XCC_ID[3:0], hwreg 20 on gfx942 / gfx950
    const unsigned long long t = __builtin_amdgcn_s_memtime(), r = __builtin_amdgcn_s_memrealtime();
    out[2 * xcc] = t;
    out[2 * xcc + 1] = r;
}
extern "C" int fmri_clock_stamp(unsigned long long* out16, fmri_stream_t stream) {
    if (!out16) return FMRI_E_SHAPE;
    k_clock_stamp<<<64, 64, 0, as_stream(stream)>>>(out16);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

__device__ __forceinline__ void decode_vox(int64_t v, int Do, int Ho, int Wo, int& n, int& d, int& h, int& w) {
    w = (int)(v % Wo); v /= Wo;
    h = (int)(v % Ho); v /= Ho;
    d = (int)(v % Do);
    n = (int)(v / Do);
}

// ------------------------------------------------------------------------------------------------ max-pool / nearest up-sampling
// MaxPooling3D(pool_size) / UpSampling3D(size) of the reference's builders (unet3d/unet.py:51, :138) with per-axis factors 1..4, stride =
// window: 2x2x2, (2, 2, 1) for the anisotropic fetal volumes or, planar, MaxPooling2D / UpSampling2D as (1, ph, pw).  Every fine voxel
// belongs to exactly one window, so one thread (one channel vector of VEC) owns a window and writes all of its children - no atomics.
// The window PD x PH x PW is a template argument: 2x2x2 and 1x2x2 (the training step's) are walked by fully unrolled loops, PD = 0 takes
// the window from PoolDims and walks it by run-time loops.  Every instantiation visits a window in (d, h, w) scan order: one
// first-maximum rule, one fp32 summation order.
struct PoolDims {
    int D, H, W;          // coarse dims
    int pd, ph, pw;
};
template <int PD, int PH, int PW>
__device__ __forceinline__ PoolDims with_window(PoolDims p) {
    if (PD > 0) { p.pd = PD; p.ph = PH; p.pw = PW; }
    return p;
}
__device__ __forceinline__ int64_t fine_vox(const PoolDims& p, int n, int d, int h, int w, int a, int b, int c) {
    return (((int64_t)n * (p.D * p.pd) + d * p.pd + a) * (p.H * p.ph) + h * p.ph + b) * (p.W * p.pw) + w * p.pw + c;
}
// f(a, b, c) for every voxel of the window, in (d, h, w) scan order
template <int PD, int PH, int PW, typename F>
__device__ __forceinline__ void for_window(const PoolDims& p, F f) {
    if constexpr (PD > 0) {
#pragma unroll
        for (int a = 0; a < PD; ++a)
#pragma unroll
            for (int b = 0; b < PH; ++b)
#pragma unroll
                for (int c = 0; c < PW; ++c) f(a, b, c);
    } else {
        for (int a = 0; a < p.pd; ++a)
            for (int b = 0; b < p.ph; ++b)
                for (int c = 0; c < p.pw; ++c) f(a, b, c);
    }
}

template <typename T, int VEC, int PD, int PH, int PW>
__global__ void __launch_bounds__(256) k_maxpool_fwd(const T* __restrict__ x, T* __restrict__ y, int N, int C, PoolDims pr) {
    const PoolDims p = with_window<PD, PH, PW>(pr);
    const int CG = C / VEC;
    const int64_t total = (int64_t)N * p.D * p.H * p.W * CG;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int cg = (int)(i % CG), n, d, h, w;
        decode_vox(i / CG, p.D, p.H, p.W, n, d, h, w);
        float m[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) m[k] = -INFINITY;
        for_window<PD, PH, PW>(p, [&](int a, int b, int c) {
            float xv[VEC];
            ldv<T, VEC>(x + fine_vox(p, n, d, h, w, a, b, c) * C + cg * VEC, xv);
#pragma unroll
            for (int k = 0; k < VEC; ++k) m[k] = fmaxf(m[k], xv[k]);
        });
        stv<T, VEC>(y + (i / CG) * C + cg * VEC, m);
    }
}

// backward: the window's maximum, then dy to the FIRST maximum in scan order, + the skip gradient, the producer's ReLU mask, every child
// written.  A fixed window of at most 8 voxels keeps its values and offsets in registers and reads x once; any other window is too large
// for that (4x4x4 is 64 voxels) and reads x twice - find the maximum, then route.
template <typename T, int VEC, int PD, int PH, int PW>
__global__ void __launch_bounds__(256) k_maxpool_bwd(const T* __restrict__ x, const T* __restrict__ dy, const T* __restrict__ add, int add_ld,
                                                     int add_off, T* __restrict__ dx, int N, int C, int relu_mask, PoolDims pr) {
    constexpr int NT = PD * PH * PW;
    constexpr bool IN_REGS = NT >= 1 && NT <= 8;
    const PoolDims p = with_window<PD, PH, PW>(pr);
    const int CG = C / VEC;
    const int64_t total = (int64_t)N * p.D * p.H * p.W * CG;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int cg = (int)(i % CG), n, d, h, w;
        decode_vox(i / CG, p.D, p.H, p.W, n, d, h, w);
        float m[VEC], g[VEC];
        bool taken[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) { m[k] = -INFINITY; taken[k] = false; }
        // the gradient of fine voxel v (its values xv).  A macro, not a lambda: a closure that captures `taken` moves those flags from
        // wave masks into vector registers in the run-time instantiation, which then is no longer the code that was measured
#define ROUTE(v, xv)                                                                           \
    do {                                                                                       \
        float r[VEC], s[VEC];                                                                  \
        if (add) ldv<T, VEC>(add + (v) * add_ld + add_off + cg * VEC, s);                      \
        _Pragma("unroll") for (int k = 0; k < VEC; ++k) {                                      \
            float rr = 0.f;                                                                    \
            if (!taken[k] && (xv)[k] == m[k]) { rr = g[k]; taken[k] = true; }                  \
            if (add) rr += s[k];                                                               \
            if (relu_mask && !((xv)[k] > 0.f)) rr = 0.f;                                       \
            r[k] = rr;                                                                         \
        }                                                                                      \
        stv<T, VEC>(dx + (v) * C + cg * VEC, r);                                               \
    } while (0)
        if constexpr (IN_REGS) {
            float xw[NT][VEC];
            int64_t vw[NT];
            for_window<PD, PH, PW>(p, [&](int a, int b, int c) {
                const int t = (a * PH + b) * PW + c;
                vw[t] = fine_vox(p, n, d, h, w, a, b, c);
                ldv<T, VEC>(x + vw[t] * C + cg * VEC, xw[t]);
#pragma unroll
                for (int k = 0; k < VEC; ++k) m[k] = fmaxf(m[k], xw[t][k]);
            });
            ldv<T, VEC>(dy + (i / CG) * C + cg * VEC, g);
            for_window<PD, PH, PW>(p, [&](int a, int b, int c) {
                const int t = (a * PH + b) * PW + c;
                ROUTE(vw[t], xw[t]);
            });
        } else {
            for_window<PD, PH, PW>(p, [&](int a, int b, int c) {
                float xv[VEC];
                ldv<T, VEC>(x + fine_vox(p, n, d, h, w, a, b, c) * C + cg * VEC, xv);
#pragma unroll
                for (int k = 0; k < VEC; ++k) m[k] = fmaxf(m[k], xv[k]);
            });
            ldv<T, VEC>(dy + (i / CG) * C + cg * VEC, g);
            for (int a = 0; a < p.pd; ++a)                       // (plain loops: `taken` in no closure, see ROUTE)
                for (int b = 0; b < p.ph; ++b)
                    for (int c = 0; c < p.pw; ++c) {
                        const int64_t v = fine_vox(p, n, d, h, w, a, b, c);
                        float xv[VEC];
                        ldv<T, VEC>(x + v * C + cg * VEC, xv);
                        ROUTE(v, xv);
                    }
        }
#undef ROUTE
    }
}

// D, H, W of PoolDims = the low-resolution dims; y / dy: channel slice [off, off + C) of a tensor with ld channels
template <typename T, int VEC, int PD, int PH, int PW>
__global__ void __launch_bounds__(256) k_upsample_fwd(const T* __restrict__ x, T* __restrict__ y, int y_ld, int y_off, int N, int C, PoolDims pr) {
    const PoolDims p = with_window<PD, PH, PW>(pr);
    const int CG = C / VEC;
    const int64_t total = (int64_t)N * p.D * p.H * p.W * CG;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int cg = (int)(i % CG), n, d, h, w;
        decode_vox(i / CG, p.D, p.H, p.W, n, d, h, w);
        float v[VEC];
        ldv<T, VEC>(x + (i / CG) * C + cg * VEC, v);
        for_window<PD, PH, PW>(p, [&](int a, int b, int c) { stv<T, VEC>(y + fine_vox(p, n, d, h, w, a, b, c) * y_ld + y_off + cg * VEC, v); });
    }
}

template <typename T, int VEC, int PD, int PH, int PW>
__global__ void __launch_bounds__(256) k_upsample_bwd(const T* __restrict__ dy, int dy_ld, int dy_off, const T* __restrict__ xmask,
                                                      T* __restrict__ dx, int N, int C, PoolDims pr) {
    const PoolDims p = with_window<PD, PH, PW>(pr);
    const int CG = C / VEC;
    const int64_t total = (int64_t)N * p.D * p.H * p.W * CG;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int cg = (int)(i % CG), n, d, h, w;
        decode_vox(i / CG, p.D, p.H, p.W, n, d, h, w);
        float acc[VEC];
#pragma unroll
        for (int k = 0; k < VEC; ++k) acc[k] = 0.f;
        for_window<PD, PH, PW>(p, [&](int a, int b, int c) {
            float g[VEC];
            ldv<T, VEC>(dy + fine_vox(p, n, d, h, w, a, b, c) * dy_ld + dy_off + cg * VEC, g);
#pragma unroll
            for (int k = 0; k < VEC; ++k) acc[k] += g[k];
        });
        if (xmask) {
            float m[VEC];
            ldv<T, VEC>(xmask + (i / CG) * C + cg * VEC, m);
#pragma unroll
            for (int k = 0; k < VEC; ++k) if (!(m[k] > 0.f)) acc[k] = 0.f;
        }
        stv<T, VEC>(dx + (i / CG) * C + cg * VEC, acc);
    }
}

// factors 1..4 per axis, not all 1 (that is a copy, not a pooling layer)
static inline bool pool_factors_ok(int pd, int ph, int pw) {
    if (pd < 1 || pd > 4 || ph < 1 || ph > 4 || pw < 1 || pw > 4) return false;
    return pd * ph * pw > 1;
}

// dtype x vector width x window -> one instantiation: launch(T{}, VEC, PD, PH, PW), the last four as integral constants.  The fixed
// windows are 2x2x2 and 1x2x2; every other window is PD = 0.
template <int V> using IntC = std::integral_constant<int, V>;
template <typename F>
static int pool_dispatch(int dtype, int vec, const PoolDims& p, F launch) {
    auto by_window = [&](auto t, auto v) {
        if (p.pd == 2 && p.ph == 2 && p.pw == 2) launch(t, v, IntC<2>{}, IntC<2>{}, IntC<2>{});
        else if (p.pd == 1 && p.ph == 2 && p.pw == 2) launch(t, v, IntC<1>{}, IntC<2>{}, IntC<2>{});
        else launch(t, v, IntC<0>{}, IntC<0>{}, IntC<0>{});
    };
    auto by_vec = [&](auto t) {
        switch (vec) {
            case 8: by_window(t, IntC<8>{}); break;
            case 4: by_window(t, IntC<4>{}); break;
            case 2: by_window(t, IntC<2>{}); break;
            default: by_window(t, IntC<1>{}); break;
        }
    };
    if (dtype == FMRI_F32) by_vec(float{});
    else if (dtype == FMRI_BF16) by_vec(bf16_t{});
    else return FMRI_E_DTYPE;
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
// the `launch` of pool_dispatch for kernel KERN; its arguments cast the tensors with (T*) / (const T*)
#define POOL_LAUNCH(KERN, grid, s, ...)                                                                                              \
    [&](auto t, auto v, auto a, auto b, auto c) {                                                                                    \
        using T = decltype(t);                                                                                                       \
        KERN<T, decltype(v)::value, decltype(a)::value, decltype(b)::value, decltype(c)::value><<<grid, 256, 0, s>>>(__VA_ARGS__);   \
    }

extern "C" int fmri_maxpool3d_fwd(const void* x, void* y, int N, int D, int H, int W, int C, int pd, int ph, int pw, int dtype,
                                  fmri_stream_t stream) {
    if (N <= 0 || C <= 0 || D < 1 || H < 1 || W < 1 || !pool_factors_ok(pd, ph, pw) || D % pd || H % ph || W % pw) return FMRI_E_SHAPE;
    const PoolDims p = {D / pd, H / ph, W / pw, pd, ph, pw};
    int vec = pick_vec(C);
    int grid = grid_for((int64_t)N * p.D * p.H * p.W * (C / vec));
    return pool_dispatch(dtype, vec, p, POOL_LAUNCH(k_maxpool_fwd, grid, as_stream(stream), (const T*)x, (T*)y, N, C, p));
}

extern "C" int fmri_maxpool3d_bwd(const void* x, const void* dy, const void* add, int add_ld, int add_off, void* dx, int N, int D, int H,
                                  int W, int C, int pd, int ph, int pw, int relu_mask, int dtype, fmri_stream_t stream) {
    if (N <= 0 || C <= 0 || D < 1 || H < 1 || W < 1 || !pool_factors_ok(pd, ph, pw) || D % pd || H % ph || W % pw) return FMRI_E_SHAPE;
    if (add && (add_off < 0 || add_ld < add_off + C)) return FMRI_E_SHAPE;
    const PoolDims p = {D / pd, H / ph, W / pw, pd, ph, pw};
    int vec = pick_vec(C);
    if (add) { while (vec > 1 && ((add_ld % vec) || (add_off % vec))) vec >>= 1; }
    int grid = grid_for((int64_t)N * p.D * p.H * p.W * (C / vec));
    return pool_dispatch(dtype, vec, p, POOL_LAUNCH(k_maxpool_bwd, grid, as_stream(stream), (const T*)x, (const T*)dy, (const T*)add, add_ld,
                                                    add_off, (T*)dx, N, C, relu_mask, p));
}

extern "C" int fmri_upsample_nearest_fwd(const void* x, void* y, int y_ld, int y_off, int N, int D, int H, int W, int C, int pd, int ph,
                                         int pw, int dtype, fmri_stream_t stream) {
    if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || !pool_factors_ok(pd, ph, pw) || y_off < 0 || y_ld < y_off + C) return FMRI_E_SHAPE;
    const PoolDims p = {D, H, W, pd, ph, pw};
    int vec = pick_vec(C);
    while (vec > 1 && ((y_ld % vec) || (y_off % vec))) vec >>= 1;
    int grid = grid_for((int64_t)N * D * H * W * (C / vec));
    return pool_dispatch(dtype, vec, p, POOL_LAUNCH(k_upsample_fwd, grid, as_stream(stream), (const T*)x, (T*)y, y_ld, y_off, N, C, p));
}

extern "C" int fmri_upsample_nearest_bwd(const void* dy, int dy_ld, int dy_off, const void* xmask, void* dx, int N, int D, int H, int W,
                                         int C, int pd, int ph, int pw, int dtype, fmri_stream_t stream) {
    if (N <= 0 || C <= 0 || D <= 0 || H <= 0 || W <= 0 || !pool_factors_ok(pd, ph, pw) || dy_off < 0 || dy_ld < dy_off + C) return FMRI_E_SHAPE;
    const PoolDims p = {D, H, W, pd, ph, pw};
    int vec = pick_vec(C);
    while (vec > 1 && ((dy_ld % vec) || (dy_off % vec))) vec >>= 1;
    int grid = grid_for((int64_t)N * D * H * W * (C / vec));
    return pool_dispatch(dtype, vec, p, POOL_LAUNCH(k_upsample_bwd, grid, as_stream(stream), (const T*)dy, dy_ld, dy_off, (const T*)xmask,
                                                    (T*)dx, N, C, p));
}

// ------------------------------------------------------------------------------------------------ final 1x1x1 conv
// Reference: Conv3D(n_labels,(1,1,1)) at unet3d/unet.py:68.  AI ~ 1 flop/B: one pass over x, C small (<= 256).
// One thread per voxel, channel loop vectorised; weights broadcast from LDS.
template <typename T, int VEC>
__global__ void k_conv1x1_fwd(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                              float* __restrict__ logits, int64_t nvox, int C, int L) {
    extern __shared__ __attribute__((aligned(16))) float sw[];  // [L][C]
    for (int i = threadIdx.x; i < L * C; i += blockDim.x) sw[i] = w[i];
    __syncthreads();
    for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < nvox; v += (int64_t)gridDim.x * blockDim.x) {
        for (int l = 0; l < L; ++l) {
            float acc = b ? b[l] : 0.f;
            for (int c = 0; c < C; c += VEC) {
                float xv[VEC];
                ldv<T, VEC>(x + v * C + c, xv);
#pragma unroll
                for (int k = 0; k < VEC; ++k) acc = fmaf(xv[k], sw[l * C + c + k], acc);
            }
            logits[v * L + l] = acc;
        }
    }
}
// backward: dx (masked), and block-reduced dw/db with one atomic per (block, output).
template <typename T, int VEC>
__global__ void k_conv1x1_bwd(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dl,
                              T* __restrict__ dx, float* __restrict__ dw, float* __restrict__ db, int64_t nvox, int C, int L,
                              int relu_mask) {
    extern __shared__ __attribute__((aligned(16))) float sm[];  // [L][C] weights, then [L][C+1] accumulators
    float* sw = sm;
    float* sacc = sm + L * C;
    for (int i = threadIdx.x; i < L * C; i += blockDim.x) sw[i] = w[i];
    for (int i = threadIdx.x; i < L * (C + 1); i += blockDim.x) sacc[i] = 0.f;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    for (int64_t v0 = blockIdx.x * (int64_t)blockDim.x; v0 < nvox; v0 += (int64_t)gridDim.x * blockDim.x) {
        int64_t v = v0 + threadIdx.x;
        bool ok = v < nvox;
        for (int c = 0; c < C; c += VEC) {
            float xv[VEC], gx[VEC];
            if (ok) ldv<T, VEC>(x + v * C + c, xv);
            else {
#pragma unroll
                for (int k = 0; k < VEC; ++k) xv[k] = 0.f;
            }
#pragma unroll
            for (int k = 0; k < VEC; ++k) gx[k] = 0.f;
            for (int l = 0; l < L; ++l) {
                float g = ok ? dl[v * L + l] : 0.f;
#pragma unroll
                for (int k = 0; k < VEC; ++k) {
                    gx[k] = fmaf(g, sw[l * C + c + k], gx[k]);
                    float p = g * xv[k];  // dw contribution: wave-reduce then one LDS atomic
                    for (int o = 32; o > 0; o >>= 1) p += __shfl_down(p, o);
                    if (lane == 0) atomicAdd(&sacc[l * (C + 1) + c + k], p);
                }
            }
            if (ok && dx) {
                if (relu_mask) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) if (!(xv[k] > 0.f)) gx[k] = 0.f;
                }
                stv<T, VEC>(dx + v * C + c, gx);
            }
        }
        for (int l = 0; l < L; ++l) {
            float g = ok ? dl[v * L + l] : 0.f;
            for (int o = 32; o > 0; o >>= 1) g += __shfl_down(g, o);
            if (lane == 0) atomicAdd(&sacc[l * (C + 1) + C], g);
        }
    }
    __syncthreads();
    const FmriDetCfg dc = g_det_cfg;
    for (int i = threadIdx.x; i < L * (C + 1); i += blockDim.x) {
        int l = i / (C + 1), c = i % (C + 1);
        if (c < C) fmri_grad_add(dc, &dw[l * C + c], sacc[i]);
        else if (db) fmri_grad_add(dc, &db[l], sacc[i]);
    }
}


// ---- fast path: LPV = C/8 lanes cooperate on one voxel (16-B loads, whole 128-B lines per voxel group), L <= 4.
template <typename T, int LPV>
__global__ void __launch_bounds__(256)
k_conv1x1_fwd_v2(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ logits,
                 int64_t nvox, int C, int L) {
    const int sub = threadIdx.x % LPV;                 // which 8-channel group of the voxel
    float wr[4][8];
#pragma unroll
    for (int l = 0; l < 4; ++l)
#pragma unroll
        for (int k = 0; k < 8; ++k) wr[l][k] = l < L ? w[l * C + sub * 8 + k] : 0.f;
    const int64_t vpb = blockDim.x / LPV;
    for (int64_t v = blockIdx.x * vpb + threadIdx.x / LPV; v < nvox + (vpb - 1); v += (int64_t)gridDim.x * vpb) {
        const bool ok = v < nvox;                      // keep whole waves in the shuffles
        float xv[8];
        if (ok) ldv<T, 8>(x + v * C + sub * 8, xv);
        else {
#pragma unroll
            for (int k = 0; k < 8; ++k) xv[k] = 0.f;
        }
#pragma unroll
        for (int l = 0; l < 4; ++l) {
            if (l < L) {
                float a = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) a = fmaf(xv[k], wr[l][k], a);
#pragma unroll
                for (int o = LPV / 2; o > 0; o >>= 1) a += __shfl_xor(a, o);
                if (ok && sub == 0) logits[v * L + l] = a + (b ? b[l] : 0.f);
            }
        }
    }
}
template <typename T, int LPV>
__global__ void __launch_bounds__(256)
k_conv1x1_bwd_v2(const T* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dl, T* __restrict__ dx,
                 float* __restrict__ dw, float* __restrict__ db, int64_t nvox, int C, int L, int relu_mask) {
    // [L][C+1] sums of the workgroup in 2^-40 fixed point: 64-bit integer adds give the same bits in any order (fp32 LDS atomics from 32
    // voxel lanes per element did not: the workgroup's partial sums - and with them dw of the last layer - differed from run to run)
    extern __shared__ __attribute__((aligned(16))) unsigned long long sacc[];
    for (int i = threadIdx.x; i < L * (C + 1); i += blockDim.x) sacc[i] = 0ull;
    __syncthreads();
    const int sub = threadIdx.x % LPV;
    float wr[4][8], aw[4][8], ab[4];
#pragma unroll
    for (int l = 0; l < 4; ++l) {
        ab[l] = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { wr[l][k] = l < L ? w[l * C + sub * 8 + k] : 0.f; aw[l][k] = 0.f; }
    }
    const int64_t vpb = blockDim.x / LPV;
    const int64_t stride = (int64_t)gridDim.x * vpb;
    // four voxels per trip: their loads are issued together (HBM-bound kernel: one dependent load per trip left the memory pipe half empty)
    for (int64_t v0 = blockIdx.x * vpb + threadIdx.x / LPV; v0 < nvox; v0 += 4 * stride) {
        float xv[4][8];
        float gl[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t v = v0 + u * stride;
            if (v < nvox) {
                ldv<T, 8>(x + v * C + sub * 8, xv[u]);
#pragma unroll
                for (int l = 0; l < 4; ++l) gl[u][l] = l < L ? dl[v * L + l] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t v = v0 + u * stride;
            if (v >= nvox) break;
            float gx[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) gx[k] = 0.f;
#pragma unroll
            for (int l = 0; l < 4; ++l) {
                if (l < L) {
                    const float g = gl[u][l];
                    ab[l] += g;
#pragma unroll
                    for (int k = 0; k < 8; ++k) { gx[k] = fmaf(g, wr[l][k], gx[k]); aw[l][k] = fmaf(g, xv[u][k], aw[l][k]); }
                }
            }
            if (dx) {
                if (relu_mask) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) if (!(xv[u][k] > 0.f)) gx[k] = 0.f;
                }
                stv<T, 8>(dx + v * C + sub * 8, gx);
            }
        }
    }
    for (int l = 0; l < L; ++l) {
#pragma unroll
        for (int k = 0; k < 8; ++k) atomicAdd(&sacc[l * (C + 1) + sub * 8 + k], (unsigned long long)__float2ll_rn(aw[l][k] * FMRI_DET_SCALE));
        if (sub == 0) atomicAdd(&sacc[l * (C + 1) + C], (unsigned long long)__float2ll_rn(ab[l] * FMRI_DET_SCALE));
    }
    __syncthreads();
    const FmriDetCfg dc = g_det_cfg;
    for (int i = threadIdx.x; i < L * (C + 1); i += blockDim.x) {
        int l = i / (C + 1), c = i % (C + 1);
        const float v = (float)((double)(long long)sacc[i] * (1.0 / (double)FMRI_DET_SCALE));
        if (c < C) fmri_grad_add(dc, &dw[l * C + c], v);
        else if (db) fmri_grad_add(dc, &db[l], v);
    }
}
static int lpv_of(int C, int L) {
    if ((C % 8) || L > 4) return 0;
    int lpv = C / 8;
    if (lpv > 64 || (lpv & (lpv - 1))) return 0;
    return lpv;
}
#define LAUNCH_LPV(KERN, T, lpv, grid, sh, s, ...)                              \
    switch (lpv) {                                                              \
        case 1: KERN<T, 1><<<grid, 256, sh, s>>>(__VA_ARGS__); break;           \
        case 2: KERN<T, 2><<<grid, 256, sh, s>>>(__VA_ARGS__); break;           \
        case 4: KERN<T, 4><<<grid, 256, sh, s>>>(__VA_ARGS__); break;           \
        case 8: KERN<T, 8><<<grid, 256, sh, s>>>(__VA_ARGS__); break;           \
        case 16: KERN<T, 16><<<grid, 256, sh, s>>>(__VA_ARGS__); break;         \
        case 32: KERN<T, 32><<<grid, 256, sh, s>>>(__VA_ARGS__); break;         \
        default: KERN<T, 64><<<grid, 256, sh, s>>>(__VA_ARGS__); break;         \
    }

extern "C" int fmri_conv1x1_fwd(const void* x, const float* w, const float* b, float* logits, int64_t nvox, int C, int L,
                                int dtype, fmri_stream_t stream) {
    if (nvox <= 0 || C <= 0 || L <= 0 || (size_t)L * C * 4 > 64 * 1024) return FMRI_E_SHAPE;
    int vec = pick_vec(C);
    int grid = grid_for(nvox, 256, 256 * 8);
    hipStream_t s = as_stream(stream);
    size_t sh = (size_t)L * C * 4;
    if (int lpv = lpv_of(C, L)) {
        int g2 = grid_for(nvox * lpv, 256, 256 * 8);
        if (dtype == FMRI_F32) { LAUNCH_LPV(k_conv1x1_fwd_v2, float, lpv, g2, 0, s, (const float*)x, w, b, logits, nvox, C, L) }
        else if (dtype == FMRI_BF16) { LAUNCH_LPV(k_conv1x1_fwd_v2, bf16_t, lpv, g2, 0, s, (const bf16_t*)x, w, b, logits, nvox, C, L) }
        else return FMRI_E_DTYPE;
        FMRI_LAUNCH_CHECK();
        return FMRI_OK;
    }
    if (dtype == FMRI_F32) {
        switch (vec) {
            case 8: k_conv1x1_fwd<float, 8><<<grid, 256, sh, s>>>((const float*)x, w, b, logits, nvox, C, L); break;
            case 4: k_conv1x1_fwd<float, 4><<<grid, 256, sh, s>>>((const float*)x, w, b, logits, nvox, C, L); break;
            case 2: k_conv1x1_fwd<float, 2><<<grid, 256, sh, s>>>((const float*)x, w, b, logits, nvox, C, L); break;
            default: k_conv1x1_fwd<float, 1><<<grid, 256, sh, s>>>((const float*)x, w, b, logits, nvox, C, L); break;
        }
    } else if (dtype == FMRI_BF16) {
        switch (vec) {
            case 8: k_conv1x1_fwd<bf16_t, 8><<<grid, 256, sh, s>>>((const bf16_t*)x, w, b, logits, nvox, C, L); break;
            case 4: k_conv1x1_fwd<bf16_t, 4><<<grid, 256, sh, s>>>((const bf16_t*)x, w, b, logits, nvox, C, L); break;
            case 2: k_conv1x1_fwd<bf16_t, 2><<<grid, 256, sh, s>>>((const bf16_t*)x, w, b, logits, nvox, C, L); break;
            default: k_conv1x1_fwd<bf16_t, 1><<<grid, 256, sh, s>>>((const bf16_t*)x, w, b, logits, nvox, C, L); break;
        }
    } else return FMRI_E_DTYPE;
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_conv1x1_bwd(const void* x, const float* w, const float* dlogits, void* dx, float* dw, float* db,
                                int64_t nvox, int C, int L, int relu_mask, int dtype, fmri_stream_t stream) {
    if (nvox <= 0 || C <= 0 || L <= 0 || (size_t)L * (2 * C + 1) * 4 > 64 * 1024) return FMRI_E_SHAPE;
    int vec = pick_vec(C, 4);
    int grid = grid_for(nvox, 256, 256 * 4);
    hipStream_t s = as_stream(stream);
    size_t sh = (size_t)L * (2 * C + 1) * 4;
    if (int lpv = lpv_of(C, L)) {
        // two workgroups per CU (256 CUs): every workgroup ends with L x (C + 1) LDS + global atomics and starts with an LDS clear, and the
        // streaming part wants few, long-running workgroups - measured on the benchmark's 4 x 64 x 128 x 128 x 64 tensor (ms per launch):
        // 256 workgroups 0.39, 512 0.22, 768 0.29, 1024 0.23, 2048 0.26, 4096 (the former cap) 0.31, 8192 0.35
        int g2 = grid_for(nvox * lpv, 256, 512);
        size_t sh2 = (size_t)L * (C + 1) * 8;
        if (dtype == FMRI_F32) { LAUNCH_LPV(k_conv1x1_bwd_v2, float, lpv, g2, sh2, s, (const float*)x, w, dlogits, (float*)dx, dw, db, nvox, C, L, relu_mask) }
        else if (dtype == FMRI_BF16) { LAUNCH_LPV(k_conv1x1_bwd_v2, bf16_t, lpv, g2, sh2, s, (const bf16_t*)x, w, dlogits, (bf16_t*)dx, dw, db, nvox, C, L, relu_mask) }
        else return FMRI_E_DTYPE;
        FMRI_LAUNCH_CHECK();
        return FMRI_OK;
    }
    if (dtype == FMRI_F32) {
        switch (vec) {
            case 4: k_conv1x1_bwd<float, 4><<<grid, 256, sh, s>>>((const float*)x, w, dlogits, (float*)dx, dw, db, nvox, C, L, relu_mask); break;
            case 2: k_conv1x1_bwd<float, 2><<<grid, 256, sh, s>>>((const float*)x, w, dlogits, (float*)dx, dw, db, nvox, C, L, relu_mask); break;
            default: k_conv1x1_bwd<float, 1><<<grid, 256, sh, s>>>((const float*)x, w, dlogits, (float*)dx, dw, db, nvox, C, L, relu_mask); break;
        }
    } else if (dtype == FMRI_BF16) {
        switch (vec) {
            case 4: k_conv1x1_bwd<bf16_t, 4><<<grid, 256, sh, s>>>((const bf16_t*)x, w, dlogits, (bf16_t*)dx, dw, db, nvox, C, L, relu_mask); break;
            case 2: k_conv1x1_bwd<bf16_t, 2><<<grid, 256, sh, s>>>((const bf16_t*)x, w, dlogits, (bf16_t*)dx, dw, db, nvox, C, L, relu_mask); break;
            default: k_conv1x1_bwd<bf16_t, 1><<<grid, 256, sh, s>>>((const bf16_t*)x, w, dlogits, (bf16_t*)dx, dw, db, nvox, C, L, relu_mask); break;
        }
    } else return FMRI_E_DTYPE;
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ------------------------------------------------------------------------------------------------ sigmoid + Dice
// Reference: Activation('sigmoid') unet.py:69; dice_coefficient metrics.py:11-15; vod_coefficient :18-28;
// Keras 'binary_accuracy' (unet.py:81).  Block-reduce in double, one atomic per block and sum.
__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    return v;
}
// VEC = 4: 16-byte loads of logits / weights / probabilities, 4-byte loads of the labels (the launcher checks alignment and n % 4); at most 512
// workgroups, each ending in nine double atomics on one 128-byte line (4 x 64x128x128 logits, per launch: scalar loads + 1,024 workgroups
// 27.6 us; this form with 128 / 256 / 512 / 1,024 workgroups 38.6 / 25.0 / 20.5 / 22.8 us - profiles/r06_dice_kernel_ab.log; the same sums).
template <int VEC>
__global__ void __launch_bounds__(256) k_sigmoid_dice_fwd(const float* __restrict__ logits, const uint8_t* __restrict__ y, const float* __restrict__ wgt,
                                   float* __restrict__ probs, double* __restrict__ sums, int64_t n) {
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    auto one = [&](float z, float t, float w, float& p_out) {
        float p = 1.f / (1.f + __expf(-z));
        p_out = p;
        {   // binary cross-entropy with Keras' clipping, and the reference focal term (metrics.py:80-87: alpha .5, gamma 2)
            const float pc = fminf(fmaxf(p, 1e-7f), 1.f - 1e-7f);
            s[7] += (double)(w * (t > 0.5f ? -__logf(pc) : -__logf(1.f - pc)));   // weight_mask * xent (metrics.py:72-76)
            // log p and log(1 - p) differ by the logit (1 - p = p e^-z): take the logarithm whose argument stays away from 0 and add z, so that
            // the term is finite at saturated logits (p = 1.0f from z = 17 upward, where log(1 - p) = -inf; the exact value there is z / 2)
            const float lg = (z > 0.f) == (t > 0.5f) ? __logf(t > 0.5f ? p : 1.f - p) : __logf(t > 0.5f ? 1.f - p : p) + (t > 0.5f ? z : -z);
            s[8] += (double)(t > 0.5f ? -0.5f * (1.f - p) * (1.f - p) * lg : -0.5f * p * p * lg);
        }
        s[0] += (double)(t * p);
        s[1] += (double)t;
        s[2] += (double)p;
        float tb = t > 0.5f ? 1.f : 0.f, pb = p > 0.5f ? 1.f : 0.f;
        s[3] += tb * pb;
        s[4] += tb;
        s[5] += pb;
        s[6] += (rintf(p) == t) ? 1.0 : 0.0;
    };
    const int64_t nv = n / VEC;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += (int64_t)gridDim.x * blockDim.x) {
        if constexpr (VEC == 4) {
            const float4 z = reinterpret_cast<const float4*>(logits)[i];
            const uchar4 t = reinterpret_cast<const uchar4*>(y)[i];
            float4 w = make_float4(1.f, 1.f, 1.f, 1.f), p;
            if (wgt) w = reinterpret_cast<const float4*>(wgt)[i];
            one(z.x, (float)t.x, w.x, p.x);
            one(z.y, (float)t.y, w.y, p.y);
            one(z.z, (float)t.z, w.z, p.z);
            one(z.w, (float)t.w, w.w, p.w);
            if (probs) reinterpret_cast<float4*>(probs)[i] = p;
        } else {
            float p;
            one(logits[i], (float)y[i], wgt ? wgt[i] : 1.f, p);
            if (probs) probs[i] = p;
        }
    }
    __shared__ double red[9][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        double r = wave_sum(s[k]);
        if (lane == 0) red[k][wv] = r;
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        double r = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        const int k = threadIdx.x < 7 ? threadIdx.x : threadIdx.x + 1;            // [8] = sum xent, [9] = sum focal
        // deterministic mode: the workgroups' sums meet as 2^-20 fixed-point integers (g_isums), k_isums_finish adds them to `sums`
        if (g_det_cfg.base != nullptr) atomicAdd(&g_isums[k], (unsigned long long)__double2ll_rn(r * 1048576.0));
        else atomicAdd(&sums[k], r);
    }
    if (blockIdx.x == 0 && threadIdx.x == 9) atomicAdd(&sums[7], (double)n);
}
__global__ void k_isums_finish(double* __restrict__ sums) {
    const int k = threadIdx.x;
    if (k < 16) {
        const long long v = (long long)g_isums[k];
        if (v) sums[k] += (double)v * (1.0 / 1048576.0);
        g_isums[k] = 0ull;
    }
}
// gradient += shadow * 2^-40, shadow = 0 (see FmriDetCfg in common.h)
__global__ void k_det_finish(float* __restrict__ g, unsigned long long* __restrict__ shadow, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const long long v = (long long)shadow[i];
        if (v) {
            g[i] += (float)((double)v * (1.0 / (double)FMRI_DET_SCALE));
            shadow[i] = 0ull;
        }
    }
}
__global__ void k_sigmoid_dice_bwd(const float* __restrict__ probs, const uint8_t* __restrict__ y, const double* __restrict__ sums,
                                   float* __restrict__ dl, int64_t n, float smooth, float grad_scale) {
    const double I = sums[0], den = sums[1] + sums[2] + (double)smooth;
    const float a = (float)(2.0 / den);                       // coefficient of y
    const float c = (float)((2.0 * I + (double)smooth) / (den * den));
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float p = probs[i], t = (float)y[i];
        float dLdp = -(a * t - c);
        dl[i] = grad_scale * dLdp * p * (1.f - p);
    }
}
// general loss gradient w.r.t. the logits from the (global) sums: kind 0 dice, 1 mean binary cross-entropy, 2 dice + w*xent,
// 3 focal (alpha .5, gamma 2), 4 vod (smoothed IoU on probabilities), 5 double dice (-dice(y,p) + r*dice(1-y,p))
__global__ void k_sigmoid_loss_bwd(const float* __restrict__ probs, const uint8_t* __restrict__ y, const float* __restrict__ wgt,
                                   const double* __restrict__ sums, float* __restrict__ dl, int64_t n, int kind, float p0, float smooth,
                                   float grad_scale) {
    const double I = sums[0], Sy = sums[1], Sp = sums[2], nn = sums[7];
    const double den = Sy + Sp + smooth;
    const float a = (float)(2.0 / den), c = (float)((2.0 * I + smooth) / (den * den));
    const double U = Sy + Sp - I + smooth;
    const float vu = (float)(1.0 / U), vc = (float)((I + smooth) / (U * U));
    const double I2 = Sp - I, den2 = (nn - Sy) + Sp + smooth;
    const float a2 = (float)(2.0 / den2), c2 = (float)((2.0 * I2 + smooth) / (den2 * den2));
    const float invn = (float)(1.0 / nn);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float p = probs[i], t = (float)y[i];
        const float sg = p * (1.f - p);
        // Keras clips p to [1e-7, 1 - 1e-7] inside binary_crossentropy (tf.clip_by_value): no gradient passes where the clip is active
        // (k_sigmoid_bce_bwd of the discriminator does the same)
        const float xg = (p > 1e-7f && p < 1.f - 1e-7f) ? 1.f : 0.f;
        float g;                                               // dL/dlogit
        if (kind == 0) g = -(a * t - c) * sg;
        else if (kind == 1) g = xg * (wgt ? wgt[i] : 1.f) * (p - t) * invn;
        else if (kind == 2) g = -(a * t - c) * sg + p0 * xg * (wgt ? wgt[i] : 1.f) * (p - t) * invn;
        else if (kind == 3) {
            // dL/dp * p (1 - p) with the factor folded in: q^2 p log p - q^3 / 2 (t = 1, q = 1 - p) and its mirror image; u log u -> 0 as
            // u -> 0 is taken at its limit below the normal range.  (dL/dp alone is -inf at p = 1, t = 0, and inf * p (1 - p) = inf * 0 was
            // NaN there, while the gradient is 1/2; the reference's TensorFlow formula has the same singularity - DESIGN.md.)
            const float u = t > 0.5f ? p : 1.f - p, q = 1.f - u;          // u: the probability of the true class
            const float ulu = u >= 1.17549435e-38f ? u * __logf(u) : 0.f;
            g = q * q * ulu - 0.5f * q * q * q;
            if (!(t > 0.5f)) g = -g;
        } else if (kind == 4) g = -(t * vu - (1.f - t) * vc) * sg;
        else g = (-(a * t - c) + p0 * (a2 * (1.f - t) - c2)) * sg;
        dl[i] = grad_scale * g;
    }
}
// the two passes of the sigmoid losses, weight NULL or a per-voxel weight on the cross-entropy term; the entry points check their arguments
static int sigmoid_dice_fwd_launch(const float* logits, const uint8_t* y, const float* weight, float* probs, double* sums, int64_t n,
                                   fmri_stream_t stream) {
    const bool v4 = n % 4 == 0 && !((((uintptr_t)logits) | ((uintptr_t)probs) | ((uintptr_t)weight)) & 15) && !(((uintptr_t)y) & 3);
    if (v4) k_sigmoid_dice_fwd<4><<<grid_for(n / 4, 256, 512), 256, 0, as_stream(stream)>>>(logits, y, weight, probs, sums, n);
    else k_sigmoid_dice_fwd<1><<<grid_for(n, 256, 512), 256, 0, as_stream(stream)>>>(logits, y, weight, probs, sums, n);
    if (h_det_on) k_isums_finish<<<1, 64, 0, as_stream(stream)>>>(sums);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
static int sigmoid_loss_bwd_launch(const float* probs, const uint8_t* y, const float* weight, const double* sums, float* dlogits, int64_t n,
                                   int kind, float param, float smooth, float grad_scale, fmri_stream_t stream) {
    k_sigmoid_loss_bwd<<<grid_for(n, 256, 2048), 256, 0, as_stream(stream)>>>(probs, y, weight, sums, dlogits, n, kind, param, smooth, grad_scale);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_sigmoid_loss_bwd(const float* probs, const uint8_t* y_true, const double* sums, float* dlogits, int64_t n, int kind,
                                     float param, float smooth, float grad_scale, fmri_stream_t stream) {
    if (n <= 0 || kind < 0 || kind > 5) return FMRI_E_SHAPE;
    return sigmoid_loss_bwd_launch(probs, y_true, nullptr, sums, dlogits, n, kind, param, smooth, grad_scale, stream);
}
// ---- weighted_dice_coefficient_loss (reference metrics.py:39-55): Dice per (sample, label) over the voxel axes, smooth 1e-5, MEAN over the
// (sample, label) groups - the only loss whose values the reference's own tests pin (test/test_metrics.py:10-38).
// gsums [G = nsamples * L][3] doubles: sum y*p, sum y, sum p of group g = n * L + l (element (n, v, l) sits at (n * vox + v) * L + l)
__global__ void k_wdice_sums(const float* __restrict__ probs, const uint8_t* __restrict__ y, double* __restrict__ gsums, int64_t vox, int L) {
    const int n = blockIdx.y;
    const int64_t per = vox * L;
    const float* const pp = probs + (int64_t)n * per;
    const uint8_t* const yy = y + (int64_t)n * per;
    __shared__ double red[3][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int l = 0; l < L; ++l) {
        double a = 0, b = 0, c = 0;
        for (int64_t v = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; v < vox; v += (int64_t)gridDim.x * blockDim.x) {
            const float p = pp[v * L + l], t = (float)yy[v * L + l];
            a += (double)(t * p);
            b += (double)t;
            c += (double)p;
        }
        a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
        if (lane == 0) { red[0][wv] = a; red[1][wv] = b; red[2][wv] = c; }
        __syncthreads();
        if (threadIdx.x < 3) atomicAdd(&gsums[((int64_t)n * L + l) * 3 + threadIdx.x], red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
        __syncthreads();
    }
}
// sums[10] += sum_g (2 I_g + s) / (Sy_g + Sp_g + s), sums[11] += G: additive over ranks, loss = -sums[10] / sums[11]
__global__ void k_wdice_finish(const double* __restrict__ gsums, double* __restrict__ sums, int G, float smooth) {
    double acc = 0;
    for (int g = threadIdx.x; g < G; g += blockDim.x)
        acc += (2.0 * gsums[3 * g] + (double)smooth) / (gsums[3 * g + 1] + gsums[3 * g + 2] + (double)smooth);
    acc = wave_sum(acc);
    if (threadIdx.x == 0) {
        atomicAdd(&sums[10], acc);
        atomicAdd(&sums[11], (double)G);
    }
}
// dL/dlogit of -mean_g dice_g: group g's elements get -(1 / G_total) [2 y den_g - (2 I_g + s)] / den_g^2 * p (1 - p); G_total = sums[11]
__global__ void k_wdice_bwd(const float* __restrict__ probs, const uint8_t* __restrict__ y, const double* __restrict__ gsums,
                            const double* __restrict__ sums, float* __restrict__ dl, int64_t vox, int L, float smooth, float grad_scale) {
    const int n = blockIdx.y;
    const int64_t per = vox * L, base = (int64_t)n * per;
    const double invg = 1.0 / sums[11];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < per; i += (int64_t)gridDim.x * blockDim.x) {
        const int l = (int)(i % L);
        const double* const gs = gsums + ((int64_t)n * L + l) * 3;
        const double den = gs[1] + gs[2] + (double)smooth;
        const float a = (float)(2.0 / den * invg), c = (float)((2.0 * gs[0] + (double)smooth) / (den * den) * invg);
        const float p = probs[base + i], t = (float)y[base + i];
        dl[base + i] = grad_scale * -(a * t - c) * p * (1.f - p);
    }
}
extern "C" int fmri_weighted_dice_fwd(const float* probs, const uint8_t* y_true, double* gsums, double* sums, int nsamples, int64_t vox, int L,
                                      float smooth, fmri_stream_t stream) {
    if (!probs || !y_true || !gsums || !sums || nsamples <= 0 || vox <= 0 || L <= 0 || nsamples > 65535) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    const int G = nsamples * L;
    if (hipMemsetAsync(gsums, 0, (size_t)G * 3 * sizeof(double), s) != hipSuccess) return FMRI_E_LAUNCH;
    int bx = (int)((vox + 256 * 16 - 1) / (256 * 16));
    if (bx > 256) bx = 256;
    if (h_det_on) bx = 1;          // deterministic mode: one workgroup per sample, so no two workgroups meet in a group's fp64 sums
    k_wdice_sums<<<dim3(bx, nsamples), 256, 0, s>>>(probs, y_true, gsums, vox, L);
    k_wdice_finish<<<1, 64, 0, s>>>(gsums, sums, G, smooth);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_weighted_dice_bwd(const float* probs, const uint8_t* y_true, const double* gsums, const double* sums, float* dlogits,
                                      int nsamples, int64_t vox, int L, float smooth, float grad_scale, fmri_stream_t stream) {
    if (!probs || !y_true || !gsums || !sums || !dlogits || nsamples <= 0 || vox <= 0 || L <= 0 || nsamples > 65535) return FMRI_E_SHAPE;
    int bx = (int)((vox * L + 256 * 8 - 1) / (256 * 8));
    if (bx > 1024) bx = 1024;
    k_wdice_bwd<<<dim3(bx, nsamples), 256, 0, as_stream(stream)>>>(probs, y_true, gsums, sums, dlogits, vox, L, smooth, grad_scale);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
// the same two passes with a per-voxel weight on the cross-entropy term (reference metrics.py:72-76 weighted_cross_entropy_loss,
// :89-95 dice_and_xent_mask: weight = exp(-distance_mask / sigma), computed by the caller); kinds 1 and 2 use it
extern "C" int fmri_sigmoid_dice_fwd_weighted(const float* logits, const uint8_t* y_true, const float* weight, float* probs, double* sums,
                                              int64_t n, fmri_stream_t stream) {
    if (n <= 0 || !weight) return FMRI_E_SHAPE;
    return sigmoid_dice_fwd_launch(logits, y_true, weight, probs, sums, n, stream);
}
extern "C" int fmri_sigmoid_loss_bwd_weighted(const float* probs, const uint8_t* y_true, const float* weight, const double* sums,
                                              float* dlogits, int64_t n, int kind, float param, float smooth, float grad_scale,
                                              fmri_stream_t stream) {
    if (n <= 0 || !weight || (kind != 1 && kind != 2)) return FMRI_E_SHAPE;
    return sigmoid_loss_bwd_launch(probs, y_true, weight, sums, dlogits, n, kind, param, smooth, grad_scale, stream);
}

extern "C" int fmri_sigmoid_dice_fwd(const float* logits, const uint8_t* y_true, float* probs, double* sums, int64_t n,
                                     fmri_stream_t stream) {
    if (n <= 0) return FMRI_E_SHAPE;
    return sigmoid_dice_fwd_launch(logits, y_true, nullptr, probs, sums, n, stream);
}
extern "C" int fmri_sigmoid_dice_bwd(const float* probs, const uint8_t* y_true, const double* sums, float* dlogits, int64_t n,
                                     float smooth, float grad_scale, fmri_stream_t stream) {
    if (n <= 0) return FMRI_E_SHAPE;
    k_sigmoid_dice_bwd<<<grid_for(n, 256, 2048), 256, 0, as_stream(stream)>>>(probs, y_true, sums, dlogits, n, smooth, grad_scale);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ---- label-wise Dice while training (reference metrics.py:52-59, unet.py:75-80): lsums [L][3] = sum y*p, sum y, sum p per label over the
// whole batch, element i of probs / y carrying label i % L.  The grid is a multiple of L workgroups, so the grid stride is a multiple of L
// and a thread stays with ONE label: three float64 accumulators and coalesced 4-byte / 1-byte loads.  A workgroup's 256 x 3 partial sums meet in
// LDS and thread (l, q) adds the partials of label l in thread order - a fixed order, wave after wave - then one atomic per (label, sum) and
// workgroup: float64 by default; under a deterministic registration a 2^-20 fixed-point integer added to the SAME 8-byte slot, which
// k_label_sums_finish converts in place.  No per-thread array, no dynamic register indexing.
__global__ void __launch_bounds__(256) k_label_sums(const float* __restrict__ probs, const uint8_t* __restrict__ y, int64_t n, int L,
                                                    double* __restrict__ lsums) {
    __shared__ double part[3][256];
    const int64_t tid = blockIdx.x * (int64_t)256 + threadIdx.x, step = (int64_t)gridDim.x * 256;      // step % L == 0
    double a = 0, b = 0, c = 0;
    for (int64_t i = tid; i < n; i += step) {
        const float p = probs[i], t = (float)y[i];
        a += (double)(t * p);
        b += (double)t;
        c += (double)p;
    }
    part[0][threadIdx.x] = a;
    part[1][threadIdx.x] = b;
    part[2][threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x < 3 * L) {
        const int l = threadIdx.x / 3, q = threadIdx.x - 3 * l;
        const int first = (int)((l + L - (int)((blockIdx.x * (int64_t)256) % L)) % L);                // first thread of the workgroup with label l
        double r = 0;
        for (int t = first; t < 256; t += L) r += part[q][t];
        if (g_det_cfg.base != nullptr)
            atomicAdd(reinterpret_cast<unsigned long long*>(lsums) + threadIdx.x, (unsigned long long)__double2ll_rn(r * 1048576.0));
        else atomicAdd(&lsums[threadIdx.x], r);
    }
}
__global__ void k_label_sums_finish(double* __restrict__ lsums, int n3) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n3) lsums[k] = (double)(long long)reinterpret_cast<unsigned long long*>(lsums)[k] * (1.0 / 1048576.0);
}
extern "C" int fmri_label_sums(const float* probs, const uint8_t* y_true, int64_t nvox, int L, double* lsums, fmri_stream_t stream) {
    if (!probs || !y_true || !lsums || nvox <= 0 || L < 1 || L > FMRI_MAX_LABELS) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(lsums, 0, (size_t)3 * L * sizeof(double), s) != hipSuccess) return FMRI_E_LAUNCH;
    const int64_t n = nvox * L;
    const int grid = (grid_for(n, 256 * 8, 512) + L - 1) / L * L;
    k_label_sums<<<grid, 256, 0, s>>>(probs, y_true, n, L, lsums);
    if (h_det_on) k_label_sums_finish<<<1, 128, 0, s>>>(lsums, 3 * L);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ---- overlap losses from per-label sums: Tversky, focal Tversky, Generalised Dice, boundary term (not in the reference's loss table:
// Salehi et al. 2017, Abraham & Khan 2019, Sudre et al. 2017, Kervadec et al. 2019; sign convention of the reference, loss = -coefficient).
// With I_l = sum y p, Sy_l = sum y, Sp_l = sum p of label l (fmri_label_sums) and s = smooth:
//   T(I, Sy, Sp) = (I + s) / (I + alpha (Sp - I) + beta (Sy - I) + s)          alpha weighs false positives, beta false negatives
//   kind 0  Tversky              L = -T of the sums of all labels together (as dice_coefficient flattens); default s = 1
//   kind 1  focal Tversky        L = (1 - T)^(1/gamma), the same T
//   kind 2  label-mean Tversky   L = -(1/L) sum_l T_l, T_l of label l's own sums (alpha = beta = s = 1/2: label_wise_dice_coefficient)
//   kind 3  label-mean focal     L = (1/L) sum_l (1 - T_l)^(1/gamma)
//   kind 4  Generalised Dice     L = 1 - (2 sum_l w_l I_l + s) / (sum_l w_l (Sy_l + Sp_l) + s), w_l = 1 / Sy_l^2, s = 1e-5; a label absent
//           from the batch (Sy_l = 0) takes the largest weight among the labels present, all weights are 1 when none is present; the
//           weights are constants with respect to p
//   boundary term (single label, any kind): + boundary_weight * Bd / n, Bd = sum_v phi_v p_v, phi = (1 - 2 y) * dist (the distance mask
//           holds each voxel's distance to the nearest voxel of the other class: phi is negative inside, positive outside), n = sums[7]
// The focal kinds have a pole of the gradient at T = 1 (gamma > 1): the derivative -(1/gamma) u^(1/gamma - 1) is taken at
// u = max(1 - T, 1e-7); the value is max(1 - T, 0)^(1/gamma), unclamped.
// Since dI_l/dp = y and dSp_l/dp = 1, every one of them has the gradient
//   dL/dlogit[v][l] = grad_scale * (A_l y[v][l] + B_l + boundary_scale * phi_v) * p (1 - p),  A_l = dL/dI_l, B_l = dL/dSp_l.
// k_overlap_coeffs (ONE wave, lane l = label l, wave sums in a fixed order, all float64) writes coef = {A_0, B_0, ... A_{L-1}, B_{L-1},
// value, value without the boundary term}; k_overlap_loss_bwd is the streaming pass.
__device__ __forceinline__ double wave_all_sum(double v) { return __shfl(wave_sum(v), 0); }
__device__ __forceinline__ double wave_all_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_down(v, o));
    return __shfl(v, 0);
}
__global__ void __launch_bounds__(64) k_overlap_coeffs(const double* __restrict__ lsums, const double* __restrict__ sums,
                                                       const double* __restrict__ bd, double* __restrict__ coef, int L, int kind, double alpha,
                                                       double beta, double gamma, double s, double bweight) {
    const int l = threadIdx.x;
    const bool on = l < L;
    double I = on ? lsums[3 * l] : 0.0, Sy = on ? lsums[3 * l + 1] : 0.0, Sp = on ? lsums[3 * l + 2] : 0.0;
    double A = 0.0, B = 0.0, value = 0.0;
    if (kind <= 3) {
        const bool per_label = kind >= 2, focal = (kind & 1) != 0;
        if (!per_label) { I = wave_all_sum(I); Sy = wave_all_sum(Sy); Sp = wave_all_sum(Sp); }
        const double N = I + s, D = (1.0 - alpha - beta) * I + (beta * Sy + alpha * Sp) + s;       // = I + alpha (Sp - I) + beta (Sy - I) + s
        const double T = N / D;
        const double dT_dI = (D - N * (1.0 - alpha - beta)) / (D * D), dT_dSp = -alpha * N / (D * D);
        double f = -T, df = -1.0;                                         // f(T) and f'(T)
        if (focal) {
            const double u = fmax(1.0 - T, 1e-7);
            f = pow(fmax(1.0 - T, 0.0), 1.0 / gamma);
            df = -pow(u, 1.0 / gamma - 1.0) / gamma;
        }
        const double share = per_label ? 1.0 / (double)L : 1.0;
        A = share * df * dT_dI;
        B = share * df * dT_dSp;
        value = per_label ? wave_all_sum(on ? share * f : 0.0) : f;
    } else {
        const bool present = on && Sy > 0.0;
        const double wmax = wave_all_max(present ? 1.0 / (Sy * Sy) : 0.0);        // 0: no label of the batch is present
        const double w = !on ? 0.0 : wmax == 0.0 ? 1.0 : present ? 1.0 / (Sy * Sy) : wmax;
        const double num = 2.0 * wave_all_sum(w * I) + s, den = wave_all_sum(w * (Sy + Sp)) + s;
        A = -2.0 * w / den;
        B = num * w / (den * den);
        value = 1.0 - num / den;
    }
    if (on) {
        coef[2 * l] = A;
        coef[2 * l + 1] = B;
    }
    if (l == 0) {
        coef[2 * L] = value + (bd ? bweight * bd[0] / sums[7] : 0.0);
        coef[2 * L + 1] = value;
    }
}
// Streaming pass: 4 B + 1 B in (+ 4 B of the distance mask), 4 B out per element.  The grid is a multiple of L workgroups, so the grid
// stride (in elements, x VEC) is a multiple of L and a thread keeps the labels of its first trip: its VEC coefficient pairs are loaded once,
// as floats, into named registers (k_label_sums' rule: no per-thread array, no dynamic register indexing).  VEC = 4: 16-byte loads and
// stores of probs / dist / dlogits, 4-byte loads of y; the launcher checks alignment and n % 4.
template <int VEC, bool DIST>
__global__ void __launch_bounds__(256) k_overlap_loss_bwd(const float* __restrict__ probs, const uint8_t* __restrict__ y, const float* __restrict__ dist,
                                                          const double* __restrict__ coef, float* __restrict__ dl, int64_t n, int L,
                                                          float bscale, float gs) {
    const int64_t tid = blockIdx.x * (int64_t)256 + threadIdx.x, step = (int64_t)gridDim.x * 256;          // step % L == 0
    const int l0 = (int)((tid * VEC) % L);
    auto one = [&](float p, float t, float d, float a, float b) {
        float c = a * t + b;
        if constexpr (DIST) c += bscale * (1.f - 2.f * t) * d;
        return gs * c * (p * (1.f - p));
    };
    if constexpr (VEC == 4) {
        const int l1 = l0 + 1 < L ? l0 + 1 : 0, l2 = l1 + 1 < L ? l1 + 1 : 0, l3 = l2 + 1 < L ? l2 + 1 : 0;
        const float a0 = (float)coef[2 * l0], b0 = (float)coef[2 * l0 + 1], a1 = (float)coef[2 * l1], b1 = (float)coef[2 * l1 + 1];
        const float a2 = (float)coef[2 * l2], b2 = (float)coef[2 * l2 + 1], a3 = (float)coef[2 * l3], b3 = (float)coef[2 * l3 + 1];
        const int64_t nv = n / 4;
        for (int64_t i = tid; i < nv; i += step) {
            const float4 p = reinterpret_cast<const float4*>(probs)[i];
            const uchar4 t = reinterpret_cast<const uchar4*>(y)[i];
            float4 d = make_float4(0.f, 0.f, 0.f, 0.f), g;
            if constexpr (DIST) d = reinterpret_cast<const float4*>(dist)[i];
            g.x = one(p.x, (float)t.x, d.x, a0, b0);
            g.y = one(p.y, (float)t.y, d.y, a1, b1);
            g.z = one(p.z, (float)t.z, d.z, a2, b2);
            g.w = one(p.w, (float)t.w, d.w, a3, b3);
            reinterpret_cast<float4*>(dl)[i] = g;
        }
    } else {
        const float a = (float)coef[2 * l0], b = (float)coef[2 * l0 + 1];
        for (int64_t i = tid; i < n; i += step) dl[i] = one(probs[i], (float)y[i], DIST ? dist[i] : 0.f, a, b);
    }
}
// Bd = sum_v (1 - 2 y_v) dist_v p_v (single label): wave sums, four partials per workgroup in LDS, one atomic per workgroup into bd[0] -
// float64 by default, a 2^-20 fixed-point integer in the SAME 8-byte slot under a deterministic registration (k_label_sums_finish converts it)
template <int VEC>
__global__ void __launch_bounds__(256) k_boundary_sum(const float* __restrict__ probs, const uint8_t* __restrict__ y, const float* __restrict__ dist,
                                                      int64_t n, double* __restrict__ bd) {
    double acc = 0;
    const int64_t tid = blockIdx.x * (int64_t)256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
    if constexpr (VEC == 4) {
        const int64_t nv = n / 4;
        for (int64_t i = tid; i < nv; i += step) {
            const float4 p = reinterpret_cast<const float4*>(probs)[i], d = reinterpret_cast<const float4*>(dist)[i];
            const uchar4 t = reinterpret_cast<const uchar4*>(y)[i];
            acc += (double)((1.f - 2.f * (float)t.x) * d.x * p.x);
            acc += (double)((1.f - 2.f * (float)t.y) * d.y * p.y);
            acc += (double)((1.f - 2.f * (float)t.z) * d.z * p.z);
            acc += (double)((1.f - 2.f * (float)t.w) * d.w * p.w);
        }
    } else {
        for (int64_t i = tid; i < n; i += step) acc += (double)((1.f - 2.f * (float)y[i]) * dist[i] * probs[i]);
    }
    __shared__ double red[4];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double r = red[0] + red[1] + red[2] + red[3];
        if (g_det_cfg.base != nullptr)
            atomicAdd(reinterpret_cast<unsigned long long*>(bd), (unsigned long long)__double2ll_rn(r * 1048576.0));
        else atomicAdd(bd, r);
    }
}
static inline bool overlap_vec4(int64_t n, const void* a, const void* b, const void* c, const void* y) {
    return n % 4 == 0 && !((((uintptr_t)a) | ((uintptr_t)b) | ((uintptr_t)c)) & 15) && !(((uintptr_t)y) & 3);
}
extern "C" int fmri_boundary_sum(const float* probs, const uint8_t* y_true, const float* dist, int64_t nvox, double* bd, fmri_stream_t stream) {
    if (!probs || !y_true || !dist || !bd || nvox <= 0) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    if (hipMemsetAsync(bd, 0, sizeof(double), s) != hipSuccess) return FMRI_E_LAUNCH;
    if (overlap_vec4(nvox, probs, dist, nullptr, y_true)) k_boundary_sum<4><<<grid_for(nvox / 4, 256, 512), 256, 0, s>>>(probs, y_true, dist, nvox, bd);
    else k_boundary_sum<1><<<grid_for(nvox, 256, 512), 256, 0, s>>>(probs, y_true, dist, nvox, bd);
    if (h_det_on) k_label_sums_finish<<<1, 64, 0, s>>>(bd, 1);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_overlap_coeffs(const double* lsums, const double* sums, const double* bd, double* coef, int L, int kind, float alpha,
                                   float beta, float gamma, float smooth, float boundary_weight, fmri_stream_t stream) {
    if (!lsums || !sums || !coef || L < 1 || L > FMRI_MAX_LABELS || kind < 0 || kind > 4 || !(alpha >= 0.f) || !(beta >= 0.f) || !(gamma >= 1.f) ||
        (bd && L != 1))
        return FMRI_E_SHAPE;
    k_overlap_coeffs<<<1, 64, 0, as_stream(stream)>>>(lsums, sums, bd, coef, L, kind, (double)alpha, (double)beta, (double)gamma, (double)smooth,
                                                     (double)boundary_weight);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_overlap_loss_bwd(const float* probs, const uint8_t* y_true, const float* dist, const double* coef, float* dlogits,
                                     int64_t nvox, int L, float boundary_scale, float grad_scale, fmri_stream_t stream) {
    if (!probs || !y_true || !coef || !dlogits || nvox <= 0 || L < 1 || L > FMRI_MAX_LABELS || (dist && L != 1)) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    const int64_t n = nvox * L;
    const bool v4 = overlap_vec4(n, probs, dlogits, dist, y_true);
    const int grid = (grid_for(v4 ? n / 4 : n, 256, 2048) + L - 1) / L * L;
#define OVL_(V_, D_) k_overlap_loss_bwd<V_, D_><<<grid, 256, 0, s>>>(probs, y_true, dist, coef, dlogits, n, L, boundary_scale, grad_scale)
    if (v4) { if (dist) OVL_(4, true); else OVL_(4, false); }
    else { if (dist) OVL_(1, true); else OVL_(1, false); }
#undef OVL_
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ------------------------------------------------------------------------------------------------ Keras Adam / SGD / RMSprop / AMSGrad, clipping
// Reference: Adam(lr=initial_learning_rate) at unet3d/unet.py:85; Keras 2.2 update rule (epsilon outside the sqrt).  The other optimizers
// and the clipping: Keras 2.2.4 keras/optimizers.py as published (restated from the published source: no Keras was at hand to run against, so these
// formulas are parity-unpinned; tests/optimizer_restatement.py is the float64 form the kernels are tested against).
//
// The gradient every update sees (Optimizer.get_gradients, clip_norm): g = grad_scale * G[i]; with a norm (fmri_grad_sumsq's out[1],
// read from device memory) and clipnorm > 0 and norm >= clipnorm: g = g * clipnorm / norm; with clipvalue > 0: g clamped to +-clipvalue.
// A zero norm is below every clipnorm: nothing is clipped, nothing divided.
template <bool CLIP>
struct OptGrad {
    float gs, clipnorm, norm, clipvalue;
    bool by_norm;
    __device__ __forceinline__ OptGrad(float gs_, const double* gnorm, float clipnorm_, float clipvalue_)
        : gs(gs_), clipnorm(clipnorm_), norm(0.f), clipvalue(clipvalue_), by_norm(false) {
        if (CLIP && gnorm != nullptr && clipnorm > 0.f) {
            norm = (float)*gnorm;
            by_norm = norm >= clipnorm;
        }
    }
    __device__ __forceinline__ float operator()(float g) const {
        float gr = g * gs;
        if (CLIP) {
            if (by_norm) gr = gr * clipnorm / norm;
            if (clipvalue > 0.f) gr = fminf(fmaxf(gr, -clipvalue), clipvalue);
        }
        return gr;
    }
    // the same gradient in float64 (for an increment that cancels, see k_sgd)
    __device__ __forceinline__ double f64(float g) const {
        double gr = (double)g * (double)gs;
        if (CLIP) {
            if (by_norm) gr = gr * (double)clipnorm / (double)norm;
            if (clipvalue > 0.f) gr = fmin(fmax(gr, -(double)clipvalue), (double)clipvalue);
        }
        return gr;
    }
};

// SGD: v = momentum * m - lr * g; m <- v; p <- p + v, or with Nesterov p <- p + momentum * v - lr * g.  The Nesterov increment is a
// difference of two terms that cancel wherever momentum and gradient oppose each other: it is formed in float64 from the stored v and
// rounded once, so the parameter's error stays relative to the increment itself (the kernel is HBM-bound, the fp64 work is free).
template <bool CLIP, bool NESTEROV>
__global__ void k_sgd(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, int64_t n, float lr, float mom, float gs,
                      const double* __restrict__ gnorm, float clipnorm, float clipvalue) {
    const OptGrad<CLIP> grad(gs, gnorm, clipnorm, clipvalue);
    auto step = [&](float& pk, float gk, float& mk) {
        const float v = mom * mk - lr * grad(gk);
        mk = v;
        if (NESTEROV) pk = (float)((double)pk + ((double)mom * (double)v - (double)lr * grad.f64(gk)));
        else pk += v;
    };
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 pp = ((float4*)p)[i], gg = ((const float4*)g)[i], mm = ((float4*)m)[i];
        float* pa = (float*)&pp; float* ga = (float*)&gg; float* ma = (float*)&mm;
#pragma unroll
        for (int k = 0; k < 4; ++k) step(pa[k], ga[k], ma[k]);
        ((float4*)p)[i] = pp; ((float4*)m)[i] = mm;
    }
    for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        step(p[i], g[i], m[i]);
}

// RMSprop: a <- rho * a + (1 - rho) * g^2; p <- p - lr * g / (sqrt(a) + eps)
template <bool CLIP>
__global__ void k_rmsprop(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ a, int64_t n, float lr, float rho, float eps,
                          float gs, const double* __restrict__ gnorm, float clipnorm, float clipvalue) {
    const OptGrad<CLIP> grad(gs, gnorm, clipnorm, clipvalue);
    auto step = [&](float& pk, float gk, float& ak) {
        const float gr = grad(gk);
        ak = rho * ak + (1.f - rho) * gr * gr;
        pk -= lr * gr / (sqrtf(ak) + eps);
    };
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 pp = ((float4*)p)[i], gg = ((const float4*)g)[i], aa = ((float4*)a)[i];
        float* pa = (float*)&pp; float* ga = (float*)&gg; float* sa = (float*)&aa;
#pragma unroll
        for (int k = 0; k < 4; ++k) step(pa[k], ga[k], sa[k]);
        ((float4*)p)[i] = pp; ((float4*)a)[i] = aa;
    }
    for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        step(p[i], g[i], a[i]);
}

// Adam: m <- b1 * m + (1 - b1) * g; v <- b2 * v + (1 - b2) * g^2; p <- p - lr_t * m / (sqrt(v) + eps).  <false, false> is plain Adam
// (fmri_adam_step: g = grad_scale * G[i], vhat and gnorm NULL); AMS: vhat <- max(vhat, v), and sqrt(vhat) in the denominator
template <bool CLIP, bool AMS>
__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                       float* __restrict__ vhat, int64_t n, float lr_t, float b1, float b2, float eps, float gs,
                       const double* __restrict__ gnorm, float clipnorm, float clipvalue) {
    const OptGrad<CLIP> grad(gs, gnorm, clipnorm, clipvalue);
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 pp = ((float4*)p)[i], gg = ((const float4*)g)[i], mm = ((float4*)m)[i], vv = ((float4*)v)[i], hh;
        if (AMS) hh = ((float4*)vhat)[i];
        float* pa = (float*)&pp; float* ga = (float*)&gg; float* ma = (float*)&mm; float* va = (float*)&vv; float* ha = (float*)&hh;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gr = grad(ga[k]);
            ma[k] = b1 * ma[k] + (1.f - b1) * gr;
            va[k] = b2 * va[k] + (1.f - b2) * gr * gr;
            if (AMS) {
                ha[k] = fmaxf(ha[k], va[k]);
                pa[k] -= lr_t * ma[k] / (sqrtf(ha[k]) + eps);
            } else {
                pa[k] -= lr_t * ma[k] / (sqrtf(va[k]) + eps);
            }
        }
        ((float4*)p)[i] = pp; ((float4*)m)[i] = mm; ((float4*)v)[i] = vv;
        if (AMS) ((float4*)vhat)[i] = hh;
    }
    for (int64_t i = (n4 << 2) + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float gr = grad(g[i]);
        float mi = b1 * m[i] + (1.f - b1) * gr, vi = b2 * v[i] + (1.f - b2) * gr * gr;
        m[i] = mi; v[i] = vi;
        if (AMS) {
            const float hi = fmaxf(vhat[i], vi);
            vhat[i] = hi;
            p[i] -= lr_t * mi / (sqrtf(hi) + eps);
        } else {
            p[i] -= lr_t * mi / (sqrtf(vi) + eps);
        }
    }
}

// n and alignment rules of the optimizer entries; the clipping instantiation only where something clips
#define OPT_REFUSE(n, bits, all_there)                       \
    do {                                                     \
        if ((n) <= 0 || !(all_there)) return FMRI_E_SHAPE;   \
        if ((bits) & 15) return FMRI_E_ALIGN;                \
    } while (0)
static inline bool opt_clips(const double*& gnorm, float clipnorm, float clipvalue) {
    if (!(clipnorm > 0.f)) gnorm = nullptr;          // no clipnorm: the norm is not read
    return gnorm != nullptr || clipvalue > 0.f;
}

extern "C" int fmri_sgd_step(float* p, const float* g, float* m, int64_t n, float lr, float momentum, int nesterov, float grad_scale,
                             const double* gnorm, float clipnorm, float clipvalue, fmri_stream_t stream) {
    OPT_REFUSE(n, ((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m), p && g && m);
    const bool clip = opt_clips(gnorm, clipnorm, clipvalue);
    if (((uintptr_t)gnorm) & 7) return FMRI_E_ALIGN;
    const int grid = grid_for(n / 4 + 1, 256, 2048);
    hipStream_t s = as_stream(stream);
#define SGD(C, N) k_sgd<C, N><<<grid, 256, 0, s>>>(p, g, m, n, lr, momentum, grad_scale, gnorm, clipnorm, clipvalue)
    if (clip) { if (nesterov) SGD(true, true); else SGD(true, false); }
    else { if (nesterov) SGD(false, true); else SGD(false, false); }
#undef SGD
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_rmsprop_step(float* p, const float* g, float* a, int64_t n, float lr, float rho, float eps, float grad_scale,
                                 const double* gnorm, float clipnorm, float clipvalue, fmri_stream_t stream) {
    OPT_REFUSE(n, ((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)a), p && g && a);
    const bool clip = opt_clips(gnorm, clipnorm, clipvalue);
    if (((uintptr_t)gnorm) & 7) return FMRI_E_ALIGN;
    const int grid = grid_for(n / 4 + 1, 256, 2048);
    hipStream_t s = as_stream(stream);
    if (clip) k_rmsprop<true><<<grid, 256, 0, s>>>(p, g, a, n, lr, rho, eps, grad_scale, gnorm, clipnorm, clipvalue);
    else k_rmsprop<false><<<grid, 256, 0, s>>>(p, g, a, n, lr, rho, eps, grad_scale, gnorm, clipnorm, clipvalue);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr_t, float beta1, float beta2,
                              float eps, float grad_scale, fmri_stream_t stream) {
    OPT_REFUSE(n, ((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v), p && g && m && v);
    k_adam<false, false><<<grid_for(n / 4 + 1, 256, 2048), 256, 0, as_stream(stream)>>>(p, g, m, v, nullptr, n, lr_t, beta1, beta2, eps,
                                                                                        grad_scale, nullptr, 0.f, 0.f);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

extern "C" int fmri_adam_step_ex(float* p, const float* g, float* m, float* v, float* vhat, int64_t n, float lr_t, float beta1, float beta2,
                                 float eps, float grad_scale, const double* gnorm, float clipnorm, float clipvalue, fmri_stream_t stream) {
    OPT_REFUSE(n, ((uintptr_t)p) | ((uintptr_t)g) | ((uintptr_t)m) | ((uintptr_t)v) | ((uintptr_t)vhat), p && g && m && v);          // vhat may be NULL (no AMSGrad)
    const bool clip = opt_clips(gnorm, clipnorm, clipvalue);
    if (((uintptr_t)gnorm) & 7) return FMRI_E_ALIGN;
    const int grid = grid_for(n / 4 + 1, 256, 2048);
    hipStream_t s = as_stream(stream);
#define ADAM(C, A) k_adam<C, A><<<grid, 256, 0, s>>>(p, g, m, v, vhat, n, lr_t, beta1, beta2, eps, grad_scale, gnorm, clipnorm, clipvalue)
    if (clip) { if (vhat) ADAM(true, true); else ADAM(true, false); }
    else { if (vhat) ADAM(false, true); else ADAM(false, false); }
#undef ADAM
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ---- sum of squares of the scaled gradient, for clipnorm: out[0] = sum (float(grad_scale * g_i))^2 in float64, out[1] = sqrt(out[0]).
// Built like fmri_moments_f64 (postprocess.hip): a lane adds the squares of the quads q, q + lanes, q + 2 * lanes ... of its index in
// Neumaier's form, lanes combine in a fixed tree (wave by shuffles, the four waves through LDS), k_grad_sumsq_finish (one workgroup) adds
// the workgroups' partials in index order.  The grid is a function of n alone and nothing is added atomically: the same values give the
// same bits on every run and stream, which is what FMRI_DETERMINISTIC=1 asks for - there is no second route.  A float32 squared is exact
// in float64 (48 significant bits; the exponent range of float squares lies inside that of float64).
constexpr int GSQ_THREADS = 256, GSQ_WAVES = GSQ_THREADS / 64, GSQ_GRID = 2048, GSQ_QUADS = 8;     // quads per lane before the grid saturates

__global__ __launch_bounds__(GSQ_THREADS) void k_grad_sumsq_partials(const float* __restrict__ g, int64_t n, float gs,
                                                                    MomSum* __restrict__ partial) {
#pragma clang fp contract(off)
    __shared__ MomSum part[GSQ_WAVES];
    MomSum acc{0.0, 0.0};
    auto take = [&](float v) {
        const float x = gs * v;
        const double d = (double)x;
        mom_add(acc, d * d);
    };
    const int64_t quads = n >> 2, step = (int64_t)gridDim.x * GSQ_THREADS;
    for (int64_t q = (int64_t)blockIdx.x * GSQ_THREADS + threadIdx.x; q < quads; q += step) {
        const float4 v = ((const float4*)g)[q];
        take(v.x);
        take(v.y);
        take(v.z);
        take(v.w);
    }
    if (blockIdx.x == 0 && (int64_t)threadIdx.x < (n & 3)) take(g[(quads << 2) + threadIdx.x]);       // the last n % 4 elements
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {                                        // lane 0 ends with the wave's tree
        const double bs = __shfl_down(acc.s, o), bc = __shfl_down(acc.c, o);
        mom_merge(acc, bs, bc);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        MomSum t = part[0];
        for (int w = 1; w < GSQ_WAVES; ++w) mom_merge(t, part[w].s, part[w].c);
        partial[blockIdx.x] = t;
    }
}

// one workgroup: thread i combines partials i, i + 256, ... in that order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(GSQ_THREADS) void k_grad_sumsq_finish(const MomSum* __restrict__ partial, int parts, double* __restrict__ out) {
#pragma clang fp contract(off)
    __shared__ MomSum sh[GSQ_THREADS];
    MomSum acc{0.0, 0.0};
    for (int i = threadIdx.x; i < parts; i += GSQ_THREADS) mom_merge(acc, partial[i].s, partial[i].c);
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int o = GSQ_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            MomSum t = sh[threadIdx.x];
            mom_merge(t, sh[threadIdx.x + o].s, sh[threadIdx.x + o].c);
            sh[threadIdx.x] = t;
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double total = sh[0].s + sh[0].c;
        out[0] = total;
        out[1] = sqrt(total);
    }
}

extern "C" int64_t fmri_grad_sumsq_workspace_bytes(void) { return (int64_t)(GSQ_GRID * sizeof(MomSum)); }

extern "C" int fmri_grad_sumsq(const float* g, int64_t n, float grad_scale, void* workspace, double* out, fmri_stream_t stream) {
    if (!g || !workspace || !out || n <= 0) return FMRI_E_SHAPE;
    if ((((uintptr_t)g) & 15) || ((((uintptr_t)workspace) | ((uintptr_t)out)) & 7)) return FMRI_E_ALIGN;
    hipStream_t s = as_stream(stream);
    MomSum* const partial = static_cast<MomSum*>(workspace);
    const int parts = grid_for(ceil_div64(n >> 2, GSQ_QUADS), GSQ_THREADS, GSQ_GRID);       // a function of n alone
    k_grad_sumsq_partials<<<parts, GSQ_THREADS, 0, s>>>(g, n, grad_scale, partial);
    k_grad_sumsq_finish<<<1, GSQ_THREADS, 0, s>>>(partial, parts, out);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ------------------------------------------------------------------------------------------------ weight packing
// fp32 master [27][Cout][Cin] -> compute-dtype copies: forward layout and the tap-flipped transposed dgrad layout.
template <typename T>
__global__ void __launch_bounds__(256) k_pack_weights(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wd, int Cout, int Cin) {
    __shared__ T tile[64][PACK_PITCH(T)];
    pack_plain_block<T>(blockIdx.x, w, wf, wd, Cout, Cin, tile);
}
extern "C" int fmri_conv3d_pack_weights(const float* w, void* w_fwd, void* w_dgrad, int Cout, int Cin, int dtype,
                                        fmri_stream_t stream) {
    if (Cout <= 0 || Cin <= 0) return FMRI_E_SHAPE;
    const int grid = 27 * ((Cout + 63) / 64) * ((Cin + 63) / 64);
    if (dtype == FMRI_F32) k_pack_weights<float><<<grid, 256, 0, as_stream(stream)>>>(w, (float*)w_fwd, (float*)w_dgrad, Cout, Cin);
    else if (dtype == FMRI_BF16) k_pack_weights<bf16_t><<<grid, 256, 0, as_stream(stream)>>>(w, (bf16_t*)w_fwd, (bf16_t*)w_dgrad, Cout, Cin);
    else return FMRI_E_DTYPE;
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ------------------------------------------------------------------------------------------------ sliding-window tiles
// Reference: batch_iterator / get_patch_from_3d_data (prediction.py:98-114, utils/patches.py:57-72) and the
// overlap-add loop prediction.py:188-193 and the final division :210.
template <typename T>
__global__ void k_tile_gather(const float* __restrict__ vol, int X, int Y, int Z, const int32_t* __restrict__ idx, int B, int px,
                              int py, int pz, T* __restrict__ tiles) {
    const int64_t per = (int64_t)px * py * pz, total = per * B;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int b = (int)(i / per);
        int64_t r = i % per;
        int z = (int)(r % pz); r /= pz;
        int y = (int)(r % py);
        int x = (int)(r / py);
        int gx = idx[3 * b] + x, gy = idx[3 * b + 1] + y, gz = idx[3 * b + 2] + z;
        // out-of-bound corners replicate the edge (utils/patches.py:75-91, np.pad mode="edge")
        gx = min(max(gx, 0), X - 1); gy = min(max(gy, 0), Y - 1); gz = min(max(gz, 0), Z - 1);
        tiles[i] = from_f<T>(vol[((int64_t)gx * Y + gy) * Z + gz]);
    }
}
__global__ void k_tile_scatter(const float* __restrict__ pred, const int32_t* __restrict__ idx, int B, int px, int py, int pz,
                               int C, double* __restrict__ acc, int32_t* __restrict__ cnt, int X, int Y, int Z) {
    const int64_t per = (int64_t)px * py * pz, total = per * B;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int b = (int)(i / per);
        int64_t r = i % per;
        int z = (int)(r % pz); r /= pz;
        int y = (int)(r % py);
        int x = (int)(r / py);
        int gx = idx[3 * b] + x, gy = idx[3 * b + 1] + y, gz = idx[3 * b + 2] + z;
        if (gx < 0 || gy < 0 || gz < 0 || gx >= X || gy >= Y || gz >= Z) continue;
        int64_t o = ((int64_t)gx * Y + gy) * Z + gz;
        for (int c = 0; c < C; ++c) atomicAdd(&acc[o * C + c], (double)pred[i * C + c]);
        atomicAdd(&cnt[o], 1);
    }
}
// Gaussian-importance blending (nnU-Net / MONAI mode="gaussian"): the tile voxel (x, y, z) counts with w = ((double)gx[x] * (double)gy[y]) *
// (double)gz[z] - the first product is exact (two 24-bit significands), the second rounds once - acc += w * pred, wsum += w.  One thread per
// tile voxel covers its C channels; tiles of one launch overlap, so every add is a float64 atomic; 64-bit index arithmetic throughout.
__global__ void __launch_bounds__(256) k_tile_scatter_weighted(const float* __restrict__ pred, const int32_t* __restrict__ idx, int B, int px, int py,
                                                               int pz, int C, const float* __restrict__ gx, const float* __restrict__ gy,
                                                               const float* __restrict__ gz, double* __restrict__ acc,
                                                               double* __restrict__ wsum, int X, int Y, int Z) {
    const int64_t per = (int64_t)px * py * pz, total = per * B;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / per;
        int64_t r = i - b * per;
        const int64_t z = r % pz; r /= pz;
        const int64_t y = r % py;
        const int64_t x = r / py;
        const int64_t ox = (int64_t)idx[3 * b] + x, oy = (int64_t)idx[3 * b + 1] + y, oz = (int64_t)idx[3 * b + 2] + z;
        if (ox < 0 || oy < 0 || oz < 0 || ox >= X || oy >= Y || oz >= Z) continue;
        const double w = ((double)gx[x] * (double)gy[y]) * (double)gz[z];
        const int64_t o = (ox * Y + oy) * Z + oz;
        for (int64_t c = 0; c < C; ++c) atomicAdd(&acc[o * C + c], w * (double)pred[i * C + c]);
        atomicAdd(&wsum[o], w);
    }
}
// The divisor of a voxel, D = int32_t (the tile count) or double (the weight sum): not positive -> the voxel is uncovered, divide by 1.
template <typename D> __device__ __forceinline__ bool tile_divisor(D d, double* q) {
    const bool covered = d > (D)0;
    *q = covered ? (double)d : 1.0;
    return covered;
}
template <typename D>
__global__ void k_tile_finalize(const double* __restrict__ acc, const D* __restrict__ cnt, double* __restrict__ out,
                                int32_t* __restrict__ bad, int64_t nvox, int C) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x) {
        double c;
        if (!tile_divisor<D>(cnt[i], &c)) atomicAdd(bad, 1);
        for (int k = 0; k < C; ++k) out[i * C + k] = acc[i * C + k] / c;
    }
}
extern "C" int fmri_tile_gather(const float* vol, int X, int Y, int Z, const int32_t* idx, int B, int px, int py, int pz,
                                void* tiles, int dtype, fmri_stream_t stream) {
    if (B <= 0 || px <= 0 || py <= 0 || pz <= 0 || X <= 0 || Y <= 0 || Z <= 0) return FMRI_E_SHAPE;
    int grid = grid_for((int64_t)B * px * py * pz, 256, 4096);
    if (dtype == FMRI_F32) k_tile_gather<float><<<grid, 256, 0, as_stream(stream)>>>(vol, X, Y, Z, idx, B, px, py, pz, (float*)tiles);
    else if (dtype == FMRI_BF16) k_tile_gather<bf16_t><<<grid, 256, 0, as_stream(stream)>>>(vol, X, Y, Z, idx, B, px, py, pz, (bf16_t*)tiles);
    else return FMRI_E_DTYPE;
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
// Tiles of a 2-D model with previous-slice truth channels (reference prediction.py:98-114, batch_iterator): the pz image slices of a tile
// followed by aux_nz truth slices starting aux_dz slices from the tile's corner, every coordinate clamped into the volume.  One thread per
// (tile, x, y) row gathers the row's pz + aux_nz channels in chunks of 8 and stores each chunk with the widest vector the row pitch allows (SW
// bytes; the lanes of a wave cover consecutive rows, so a wave writes one contiguous span).  aux_nz = 0 gives k_tile_gather's bytes.
template <typename T, int SW>
__global__ void __launch_bounds__(256) k_tile_gather_stack(const float* __restrict__ vol, const float* __restrict__ aux, int X, int Y, int Z,
                                                           const int32_t* __restrict__ idx, int B, int px, int py, int pz, int aux_dz, int aux_nz,
                                                           T* __restrict__ tiles) {
    constexpr int CH = 8, CHB = CH * (int)sizeof(T);
    const int C = pz + aux_nz;
    const int64_t rows = (int64_t)B * px * py;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < rows; i += (int64_t)gridDim.x * blockDim.x) {
        const int b = (int)(i / ((int64_t)px * py));
        const int r = (int)(i % ((int64_t)px * py));
        const int x = r / py, y = r % py;
        const int gx = min(max(idx[3 * b] + x, 0), X - 1), gy = min(max(idx[3 * b + 1] + y, 0), Y - 1), z0 = idx[3 * b + 2];
        const int64_t col = ((int64_t)gx * Y + gy) * Z;
        unsigned char* const row = reinterpret_cast<unsigned char*>(tiles + i * C);
        for (int c0 = 0; c0 < C; c0 += CH) {
            T v[CH];
#pragma unroll
            for (int j = 0; j < CH; ++j) {
                const int c = c0 + j;
                float f = 0.f;
                if (c < pz) f = vol[col + min(max(z0 + c, 0), Z - 1)];
                else if (c < C) f = aux[col + min(max(z0 + aux_dz + (c - pz), 0), Z - 1)];
                v[j] = from_f<T>(f);
            }
            const int nb = min(CH, C - c0) * (int)sizeof(T);        // a multiple of SW (the launch picks SW from the row pitch)
            unsigned char* const dst = row + c0 * (int)sizeof(T);
            const unsigned char* const src = reinterpret_cast<const unsigned char*>(v);
#pragma unroll
            for (int q = 0; q < CHB / SW; ++q) {
                if (q * SW >= nb) break;
                if (SW == 16) { uint4 u; __builtin_memcpy(&u, src + 16 * q, 16); *reinterpret_cast<uint4*>(dst + 16 * q) = u; }
                else if (SW == 8) { uint2 u; __builtin_memcpy(&u, src + 8 * q, 8); *reinterpret_cast<uint2*>(dst + 8 * q) = u; }
                else if (SW == 4) { unsigned u; __builtin_memcpy(&u, src + 4 * q, 4); *reinterpret_cast<unsigned*>(dst + 4 * q) = u; }
                else { unsigned short u; __builtin_memcpy(&u, src + 2 * q, 2); *reinterpret_cast<unsigned short*>(dst + 2 * q) = u; }
            }
        }
    }
}
extern "C" int fmri_tile_gather_stack(const float* vol, const float* aux, int X, int Y, int Z, const int32_t* idx, int B, int px, int py, int pz,
                                      int aux_dz, int aux_nz, void* tiles, int dtype, fmri_stream_t stream) {
    if (B <= 0 || px <= 0 || py <= 0 || pz <= 0 || aux_nz < 0 || X <= 0 || Y <= 0 || Z <= 0) return FMRI_E_SHAPE;
    if (!vol || !idx || !tiles || (aux_nz > 0 && !aux)) return FMRI_E_SHAPE;
    if (dtype != FMRI_F32 && dtype != FMRI_BF16) return FMRI_E_DTYPE;
    const int esz = dtype == FMRI_F32 ? 4 : 2;
    if ((uintptr_t)tiles % esz) return FMRI_E_ALIGN;
    // store width: the largest of 16 / 8 / 4 / 2 bytes that divides both the row pitch and the base address
    const uintptr_t a = (uintptr_t)tiles | (uintptr_t)((pz + aux_nz) * esz);
    const int sw = (a & 15) == 0 ? 16 : (a & 7) == 0 ? 8 : (a & 3) == 0 ? 4 : 2;
    const int grid = grid_for((int64_t)B * px * py, 256, 4096);
#define L_(T_, SW_) k_tile_gather_stack<T_, SW_><<<grid, 256, 0, as_stream(stream)>>>(vol, aux, X, Y, Z, idx, B, px, py, pz, aux_dz, aux_nz, (T_*)tiles)
    if (dtype == FMRI_F32) {
        if (sw == 16) L_(float, 16); else if (sw == 8) L_(float, 8); else L_(float, 4);
    } else {
        if (sw == 16) L_(bf16_t, 16); else if (sw == 8) L_(bf16_t, 8); else if (sw == 4) L_(bf16_t, 4); else L_(bf16_t, 2);
    }
#undef L_
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_tile_scatter_accumulate(const float* pred, const int32_t* idx, int B, int px, int py, int pz, int C,
                                            double* acc, int32_t* cnt, int X, int Y, int Z, fmri_stream_t stream) {
    if (B <= 0 || px <= 0 || py <= 0 || pz <= 0 || C <= 0) return FMRI_E_SHAPE;
    k_tile_scatter<<<grid_for((int64_t)B * px * py * pz, 256, 4096), 256, 0, as_stream(stream)>>>(pred, idx, B, px, py, pz, C, acc, cnt, X, Y, Z);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_tile_finalize(const double* acc, const int32_t* cnt, double* out, int32_t* bad, int64_t nvox, int C,
                                  fmri_stream_t stream) {
    if (nvox <= 0 || C <= 0) return FMRI_E_SHAPE;
    k_tile_finalize<int32_t><<<grid_for(nvox, 256, 4096), 256, 0, as_stream(stream)>>>(acc, cnt, out, bad, nvox, C);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_tile_scatter_weighted(const float* pred, const int32_t* idx, int B, int px, int py, int pz, int C, const float* gx,
                                          const float* gy, const float* gz, double* acc, double* wsum, int X, int Y, int Z,
                                          fmri_stream_t stream) {
    if (!pred || !idx || !gx || !gy || !gz || !acc || !wsum) return FMRI_E_SHAPE;
    if (B <= 0 || px <= 0 || py <= 0 || pz <= 0 || C <= 0 || X <= 0 || Y <= 0 || Z <= 0) return FMRI_E_SHAPE;
    if (((((uintptr_t)pred) | ((uintptr_t)idx) | ((uintptr_t)gx) | ((uintptr_t)gy) | ((uintptr_t)gz)) & 3) ||
        ((((uintptr_t)acc) | ((uintptr_t)wsum)) & 7)) return FMRI_E_ALIGN;
    k_tile_scatter_weighted<<<grid_for((int64_t)B * px * py * pz, 256, 4096), 256, 0, as_stream(stream)>>>(pred, idx, B, px, py, pz, C, gx, gy, gz,
                                                                                                        acc, wsum, X, Y, Z);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_tile_finalize_weighted(const double* acc, const double* wsum, double* out, int32_t* bad, int64_t nvox, int C,
                                           fmri_stream_t stream) {
    if (!acc || !wsum || !out || !bad || nvox <= 0 || C <= 0) return FMRI_E_SHAPE;
    if (((((uintptr_t)acc) | ((uintptr_t)wsum) | ((uintptr_t)out)) & 7) || (((uintptr_t)bad) & 3)) return FMRI_E_ALIGN;
    k_tile_finalize<double><<<grid_for(nvox, 256, 4096), 256, 0, as_stream(stream)>>>(acc, wsum, out, bad, nvox, C);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ---- the volume stays on the device around the tile loop: mirrored / padded / cropped copies in, mirrored / cropped means out
// (reference prediction.py:65-85 predict_flips, :138-146 the two paddings, :204-208 the crop of pad_for_fit).
// Both kernels walk their OUTPUT as the flat array it is, EPT consecutive elements per thread stored as one vector (the launch picks EPT
// from the base address alone, so odd row pitches keep the wide store); the coordinates of the first element come from two divisions
// (32-bit ones while every tensor stays below 2^31 elements) and are counted up from there.  The lanes of a wave cover one contiguous
// span of the output and, mirrored or not, one contiguous span of every input row they touch.
struct FlipGeo {
    int n[3];        // extent of the un-mirrored side (pad_flip: src; finalize_flip: out)
    int a[3];        // extent of the other side (pad_flip: dst; finalize_flip: acc)
    int lo[3];
    int mask;
};
template <typename V, int NB> __device__ __forceinline__ void store_bytes(void* dst, const V* v) {
    if (NB == 16) { uint4 u; __builtin_memcpy(&u, v, 16); *reinterpret_cast<uint4*>(dst) = u; }
    else if (NB == 8) { uint2 u; __builtin_memcpy(&u, v, 8); *reinterpret_cast<uint2*>(dst) = u; }
    else { unsigned u; __builtin_memcpy(&u, v, 4); *reinterpret_cast<unsigned*>(dst) = u; }
}
// dst[o] = fill where u = o - lo leaves [0, n) on any axis, else src[m(u)], m mirroring the axes of `mask`: np.pad(np.flip(src, axes),
// ..., constant_values=fill) followed by a crop (negative lo).  (TD)value is round-to-nearest, numpy's astype.
template <typename TS, typename TD, int EPT, typename IT>
__global__ void __launch_bounds__(256) k_volume_pad_flip(const TS* __restrict__ src, TD* __restrict__ dst, FlipGeo G, TD fill, int64_t total) {
    const int64_t chunks = (total + EPT - 1) / EPT;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < chunks; t += (int64_t)gridDim.x * blockDim.x) {
        const IT i0 = (IT)(t * EPT);
        const IT r = i0 / (IT)G.a[2];
        int oz = (int)(i0 - r * (IT)G.a[2]);
        int ox = (int)(r / (IT)G.a[1]);
        int oy = (int)(r - (IT)ox * (IT)G.a[1]);
        const int left = total - t * EPT < EPT ? (int)(total - t * EPT) : EPT;
        TD v[EPT];
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            TD e = fill;
            if (j < left) {
                int ux = ox - G.lo[0], uy = oy - G.lo[1], uz = oz - G.lo[2];
                if (ux >= 0 && ux < G.n[0] && uy >= 0 && uy < G.n[1] && uz >= 0 && uz < G.n[2]) {
                    if (G.mask & 1) ux = G.n[0] - 1 - ux;
                    if (G.mask & 2) uy = G.n[1] - 1 - uy;
                    if (G.mask & 4) uz = G.n[2] - 1 - uz;
                    e = (TD)src[((IT)ux * (IT)G.n[1] + (IT)uy) * (IT)G.n[2] + (IT)uz];
                }
                if (++oz == G.a[2]) { oz = 0; if (++oy == G.a[1]) { oy = 0; ++ox; } }
            }
            v[j] = e;
        }
        TD* const d = dst + t * EPT;
        if (left == EPT) store_bytes<TD, EPT * (int)sizeof(TD)>(d, v);
        else {
#pragma unroll
            for (int j = 0; j < EPT; ++j)
                if (j < left) d[j] = v[j];
        }
    }
}
template <typename TS, typename TD, typename IT>
static void launch_volume_pad_flip(const void* src, void* dst, const FlipGeo& G, double fill, int64_t total, hipStream_t s) {
    const uintptr_t a = (uintptr_t)dst;
    const int ept = (a & 15) == 0 ? 16 / (int)sizeof(TD) : (a & 7) == 0 ? 8 / (int)sizeof(TD) : 1;
#define L_(E_) k_volume_pad_flip<TS, TD, E_, IT><<<grid_for(ceil_div64(total, E_), 256, 4096), 256, 0, s>>>((const TS*)src, (TD*)dst, G, (TD)fill, total)
    if constexpr (sizeof(TD) == 4) {
        if (ept == 4) { L_(4); return; }
    }
    if (ept == 2) L_(2); else L_(1);
#undef L_
}
extern "C" int fmri_volume_pad_flip(const void* src, int src_dtype, int X, int Y, int Z, void* dst, int dst_dtype, int OX, int OY, int OZ,
                                    const int32_t* lo, int flip_mask, double fill, fmri_stream_t stream) {
    if (!src || !dst || !lo || src == dst || X <= 0 || Y <= 0 || Z <= 0 || OX <= 0 || OY <= 0 || OZ <= 0 || (flip_mask & ~7)) return FMRI_E_SHAPE;
    for (int k = 0; k < 3; ++k)
        if (lo[k] < -(1 << 30) || lo[k] > (1 << 30)) return FMRI_E_SHAPE;
    if ((src_dtype != FMRI_F32 && src_dtype != FMRI_F64) || (dst_dtype != FMRI_F32 && dst_dtype != FMRI_F64)) return FMRI_E_DTYPE;
    if (((uintptr_t)src % (src_dtype == FMRI_F64 ? 8 : 4)) || ((uintptr_t)dst % (dst_dtype == FMRI_F64 ? 8 : 4))) return FMRI_E_ALIGN;
    const FlipGeo G = {{X, Y, Z}, {OX, OY, OZ}, {lo[0], lo[1], lo[2]}, flip_mask};
    const int64_t total = (int64_t)OX * OY * OZ, stotal = (int64_t)X * Y * Z;
    const bool small = total + 4 < ((int64_t)1 << 31) && stotal < ((int64_t)1 << 31);
    hipStream_t s = as_stream(stream);
#define D_(TS_, TD_) do { if (small) launch_volume_pad_flip<TS_, TD_, unsigned>(src, dst, G, fill, total, s); \
                          else launch_volume_pad_flip<TS_, TD_, int64_t>(src, dst, G, fill, total, s); } while (0)
    if (src_dtype == FMRI_F64) { if (dst_dtype == FMRI_F32) D_(double, float); else D_(double, double); }
    else { if (dst_dtype == FMRI_F32) D_(float, float); else D_(float, double); }
#undef D_
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
// out[g][c] = acc[a][c] / (double)cnt[a], a = lo + m(g): k_tile_finalize's division read through the mirror and the crop, so a variant's
// means land un-mirrored in the caller's slot.  A zero count divides by 1 and is counted once per voxel.
template <int EPT, typename IT, typename D>
__global__ void __launch_bounds__(256) k_tile_finalize_flip(const double* __restrict__ acc, const D* __restrict__ cnt, double* __restrict__ out,
                                                            int32_t* __restrict__ bad, FlipGeo G, int C, int64_t total) {
    const int64_t chunks = (total + EPT - 1) / EPT;
    int nbad = 0;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < chunks; t += (int64_t)gridDim.x * blockDim.x) {
        const IT i0 = (IT)(t * EPT);
        const IT vox = i0 / (IT)C;
        int c = (int)(i0 - vox * (IT)C);
        const IT r = vox / (IT)G.n[2];
        int gz = (int)(vox - r * (IT)G.n[2]);
        int gx = (int)(r / (IT)G.n[1]);
        int gy = (int)(r - (IT)gx * (IT)G.n[1]);
        const int left = total - t * EPT < EPT ? (int)(total - t * EPT) : EPT;
        double v[EPT];
#pragma unroll
        for (int j = 0; j < EPT; ++j) {
            double e = 0.0;
            if (j < left) {
                const int ax = G.lo[0] + ((G.mask & 1) ? G.n[0] - 1 - gx : gx);
                const int ay = G.lo[1] + ((G.mask & 2) ? G.n[1] - 1 - gy : gy);
                const int az = G.lo[2] + ((G.mask & 4) ? G.n[2] - 1 - gz : gz);
                const IT a = ((IT)ax * (IT)G.a[1] + (IT)ay) * (IT)G.a[2] + (IT)az;
                double n;
                if (!tile_divisor<D>(cnt[a], &n)) nbad += c == 0;
                e = acc[a * (IT)C + (IT)c] / n;
                if (++c == C) { c = 0; if (++gz == G.n[2]) { gz = 0; if (++gy == G.n[1]) { gy = 0; ++gx; } } }
            }
            v[j] = e;
        }
        double* const d = out + t * EPT;
        if (left == EPT) store_bytes<double, EPT * 8>(d, v);
        else {
#pragma unroll
            for (int j = 0; j < EPT; ++j)
                if (j < left) d[j] = v[j];
        }
    }
    if (nbad) atomicAdd(bad, nbad);
}
template <typename D>
static int tile_finalize_flip(const double* acc, const D* cnt, int AX, int AY, int AZ, int C, double* out, int X, int Y, int Z, const int32_t* lo,
                              int flip_mask, int32_t* bad, fmri_stream_t stream) {
    if (!acc || !cnt || !out || !bad || !lo || AX <= 0 || AY <= 0 || AZ <= 0 || C <= 0 || X <= 0 || Y <= 0 || Z <= 0 || (flip_mask & ~7)) return FMRI_E_SHAPE;
    const int A[3] = {AX, AY, AZ}, N[3] = {X, Y, Z};
    for (int k = 0; k < 3; ++k)
        if (lo[k] < 0 || lo[k] > A[k] - N[k]) return FMRI_E_SHAPE;          // the window [lo, lo + n) lies inside acc
    if (((((uintptr_t)acc) | ((uintptr_t)out)) & 7) || (((uintptr_t)cnt) & (sizeof(D) - 1)) || (((uintptr_t)bad) & 3)) return FMRI_E_ALIGN;
    const FlipGeo G = {{X, Y, Z}, {AX, AY, AZ}, {lo[0], lo[1], lo[2]}, flip_mask};
    const int64_t total = (int64_t)X * Y * Z * C, atotal = (int64_t)AX * AY * AZ * C;
    const bool small = total + 2 < ((int64_t)1 << 31) && atotal < ((int64_t)1 << 31);
    const bool wide = ((uintptr_t)out & 15) == 0;
    hipStream_t s = as_stream(stream);
#define L_(E_, IT_) k_tile_finalize_flip<E_, IT_, D><<<grid_for(ceil_div64(total, E_), 256, 4096), 256, 0, s>>>(acc, cnt, out, bad, G, C, total)
    if (small) { if (wide) L_(2, unsigned); else L_(1, unsigned); }
    else { if (wide) L_(2, int64_t); else L_(1, int64_t); }
#undef L_
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_tile_finalize_flip(const double* acc, const int32_t* cnt, int AX, int AY, int AZ, int C, double* out, int X, int Y, int Z,
                                       const int32_t* lo, int flip_mask, int32_t* bad, fmri_stream_t stream) {
    return tile_finalize_flip<int32_t>(acc, cnt, AX, AY, AZ, C, out, X, Y, Z, lo, flip_mask, bad, stream);
}
extern "C" int fmri_tile_finalize_flip_weighted(const double* acc, const double* wsum, int AX, int AY, int AZ, int C, double* out, int X, int Y,
                                                int Z, const int32_t* lo, int flip_mask, int32_t* bad, fmri_stream_t stream) {
    return tile_finalize_flip<double>(acc, wsum, AX, AY, AZ, C, out, X, Y, Z, lo, flip_mask, bad, stream);
}

// ---- several labels: a label map straight from the overlap-add, and training targets from a label map
// out[v] per voxel from q_c = acc[v][c] / cnt[v] (float64, fmri_tile_finalize's division).  C == 1: values[0] where q_0 > threshold
// (reference prediction.py:257); C > 1: values[k], k the FIRST index of the maximum (np.argmax), 0 where max q < threshold (:219-222).
template <typename D>
__global__ void __launch_bounds__(256) k_tile_finalize_labels(const double* __restrict__ acc, const D* __restrict__ cnt,
                                                              uint8_t* __restrict__ out, int32_t* __restrict__ bad, int64_t nvox, int C,
                                                              double threshold, FmriLabelValues V) {
    __shared__ __attribute__((aligned(4))) uint8_t vals[FMRI_MAX_LABELS];
    fmri_label_tables(V, C, vals, nullptr);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nvox; i += (int64_t)gridDim.x * blockDim.x) {
        double c;
        if (!tile_divisor<D>(cnt[i], &c)) {
            atomicAdd(bad, 1);
            out[i] = 0;
            continue;
        }
        const double* const row = acc + i * C;
        double best = row[0] / c;
        int k = 0;
        for (int j = 1; j < C; ++j) {
            const double q = row[j] / c;
            if (q > best) { best = q; k = j; }
        }
        const bool keep = C == 1 ? best > threshold : !(best < threshold);
        out[i] = keep ? vals[k] : (uint8_t)0;
    }
}
extern "C" int fmri_tile_finalize_labels(const double* acc, const int32_t* cnt, uint8_t* out, int32_t* bad, int64_t nvox, int C,
                                         double threshold, const uint8_t* values, fmri_stream_t stream) {
    FmriLabelValues V;
    if (!acc || !cnt || !out || !bad || nvox <= 0 || fmri_label_values(values, C, &V) != FMRI_OK) return FMRI_E_SHAPE;
    k_tile_finalize_labels<int32_t><<<grid_for(nvox, 256, 4096), 256, 0, as_stream(stream)>>>(acc, cnt, out, bad, nvox, C, threshold, V);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
extern "C" int fmri_tile_finalize_labels_weighted(const double* acc, const double* wsum, uint8_t* out, int32_t* bad, int64_t nvox, int C,
                                                  double threshold, const uint8_t* values, fmri_stream_t stream) {
    FmriLabelValues V;
    if (!acc || !wsum || !out || !bad || nvox <= 0 || fmri_label_values(values, C, &V) != FMRI_OK) return FMRI_E_SHAPE;
    if (((((uintptr_t)acc) | ((uintptr_t)wsum)) & 7) || (((uintptr_t)bad) & 3)) return FMRI_E_ALIGN;
    k_tile_finalize_labels<double><<<grid_for(nvox, 256, 4096), 256, 0, as_stream(stream)>>>(acc, wsum, out, bad, nvox, C, threshold, V);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
// out[v][l] = (lab[v] == values[l]), channels last.  ROW: L is 1, 2, 4 or 8 and `out` is L-byte aligned - one thread per voxel, the row is one
// store of L bytes (the set byte is a shift of the label's index).  Otherwise the output is written as the flat byte array it is, 8 bytes
// per thread in one store (the byte at j belongs to voxel j / L, label j % L: one division per thread, then counted up), the bytes past
// the last multiple of 8 one by one.  The label bytes are read through the 256-entry value -> index table in LDS.
template <typename W>
__global__ void __launch_bounds__(256) k_labels_expand_row(const uint8_t* __restrict__ lab, int64_t n, int L, W* __restrict__ out, FmriLabelValues V) {
    __shared__ __attribute__((aligned(4))) uint8_t vals[FMRI_MAX_LABELS];
    __shared__ uint8_t lut[256];
    fmri_label_tables(V, L, vals, lut);
    for (int64_t v = blockIdx.x * (int64_t)256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
        const int k = lut[lab[v]];
        out[v] = k ? (W)((W)1 << (8 * (k - 1))) : (W)0;
    }
}
__global__ void __launch_bounds__(256) k_labels_expand_flat(const uint8_t* __restrict__ lab, int64_t n, int L, uint8_t* __restrict__ out,
                                                            int64_t words, FmriLabelValues V) {
    __shared__ __attribute__((aligned(4))) uint8_t vals[FMRI_MAX_LABELS];
    __shared__ uint8_t lut[256];
    fmri_label_tables(V, L, vals, lut);
    const int64_t tid = blockIdx.x * (int64_t)256 + threadIdx.x, step = (int64_t)gridDim.x * 256, total = n * L;
    for (int64_t t = tid; t < words; t += step) {
        int64_t v = (t * 8) / L;
        int l = (int)(t * 8 - v * L);
        int k = lut[lab[v]];
        unsigned long long w = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            w |= (unsigned long long)(k == l + 1) << (8 * j);
            if (++l == L) {
                l = 0;
                ++v;
                if (j < 7) k = lut[lab[v]];           // (v < n: byte t * 8 + j + 1 exists, the word lies below n * L)
            }
        }
        reinterpret_cast<unsigned long long*>(out)[t] = w;
    }
    for (int64_t j = words * 8 + tid; j < total; j += step) {
        const int64_t v = j / L;
        out[j] = lut[lab[v]] == (int)(j - v * L) + 1;
    }
}
extern "C" int fmri_labels_expand_u8(const uint8_t* lab, int64_t n, const uint8_t* values, int L, uint8_t* out, fmri_stream_t stream) {
    FmriLabelValues V;
    if (!lab || !out || n <= 0 || fmri_label_values(values, L, &V) != FMRI_OK) return FMRI_E_SHAPE;
    hipStream_t s = as_stream(stream);
    const bool row = (L == 1 || L == 2 || L == 4 || L == 8) && (reinterpret_cast<uintptr_t>(out) % L) == 0;
    if (row) {
        const int grid = grid_for(n, 256, 4096);
        if (L == 1) k_labels_expand_row<uint8_t><<<grid, 256, 0, s>>>(lab, n, L, out, V);
        else if (L == 2) k_labels_expand_row<uint16_t><<<grid, 256, 0, s>>>(lab, n, L, reinterpret_cast<uint16_t*>(out), V);
        else if (L == 4) k_labels_expand_row<uint32_t><<<grid, 256, 0, s>>>(lab, n, L, reinterpret_cast<uint32_t*>(out), V);
        else k_labels_expand_row<unsigned long long><<<grid, 256, 0, s>>>(lab, n, L, reinterpret_cast<unsigned long long*>(out), V);
    } else {
        const int64_t words = (reinterpret_cast<uintptr_t>(out) & 7u) == 0 ? n * L / 8 : 0;
        k_labels_expand_flat<<<grid_for(words ? words : n * L, 256, 4096), 256, 0, s>>>(lab, n, L, out, words, V);
    }
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ------------------------------------------------------------------------------------------------ casts
template <typename S, typename Dd>
__global__ void k_cast(const S* __restrict__ s, Dd* __restrict__ d, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        d[i] = from_f<Dd>(to_f<S>(s[i]));
}
extern "C" int fmri_cast(const void* src, int sd, void* dst, int dd, int64_t n, fmri_stream_t stream) {
    if (n <= 0) return FMRI_E_SHAPE;
    int grid = grid_for(n, 256, 4096);
    hipStream_t s = as_stream(stream);
    if (sd == FMRI_F32 && dd == FMRI_BF16) k_cast<float, bf16_t><<<grid, 256, 0, s>>>((const float*)src, (bf16_t*)dst, n);
    else if (sd == FMRI_BF16 && dd == FMRI_F32) k_cast<bf16_t, float><<<grid, 256, 0, s>>>((const bf16_t*)src, (float*)dst, n);
    else if (sd == FMRI_F32 && dd == FMRI_F32) k_cast<float, float><<<grid, 256, 0, s>>>((const float*)src, (float*)dst, n);
    else if (sd == FMRI_BF16 && dd == FMRI_BF16) k_cast<bf16_t, bf16_t><<<grid, 256, 0, s>>>((const bf16_t*)src, (bf16_t*)dst, n);
    else return FMRI_E_DTYPE;
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}

// ---- deterministic mode (common.h, FmriDetCfg)
int fmri_det_set_mfma(const FmriDetCfg&);
int fmri_det_set_first(const FmriDetCfg&);
int fmri_det_set_generic(const FmriDetCfg&);
int fmri_det_set_direct(const FmriDetCfg&);
int fmri_det_set_norm(const FmriDetCfg&);
extern "C" int fmri_set_deterministic(float* grad_base, void* shadow_i64, int64_t n) {
    if ((grad_base == nullptr) != (shadow_i64 == nullptr) || (grad_base && n <= 0)) return FMRI_E_SHAPE;
    const FmriDetCfg c{grad_base, (unsigned long long*)shadow_i64, grad_base ? (long long)n : 0};
    int rc = fmri_det_set_pointwise(c);
    if (!rc) rc = fmri_det_set_mfma(c);
    if (!rc) rc = fmri_det_set_first(c);
    if (!rc) rc = fmri_det_set_generic(c);
    if (!rc) rc = fmri_det_set_direct(c);
    if (!rc) rc = fmri_det_set_norm(c);
    return rc;
}
extern "C" int fmri_deterministic_finish(float* grad_base, void* shadow_i64, int64_t n, fmri_stream_t stream) {
    if (!grad_base || !shadow_i64 || n <= 0) return FMRI_E_SHAPE;
    k_det_finish<<<grid_for(n, 256, 2048), 256, 0, as_stream(stream)>>>(grad_base, (unsigned long long*)shadow_i64, n);
    FMRI_LAUNCH_CHECK();
    return FMRI_OK;
}
