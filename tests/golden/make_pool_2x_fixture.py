#!/usr/bin/env python3
"""Writes tests/golden/pool_2x_digests.json: the sha256 of every output of the retired 2x pooling / up-sampling entry points
(fmri_maxpool3d_2x_fwd / _bwd, fmri_upsample_nearest2x_fwd / _bwd) and of three fmri_adam_step steps, keyed by case.

NEEDS A LIBRARY FROM THE LAST COMMIT THAT HAS THE 2x ENTRIES (the parent of the commit that merged them into the per-axis entries); the
library of a later commit has no such symbols and this script fails at once.  Needs the GPU.

    FMRI_LIB=<checkout of that commit>/fetal-mri-segmentation_amd/lib/libfmri_hip.so python tests/golden/make_pool_2x_fixture.py [out.json]

The inputs come from an integer formula (`formula`), not from a library generator, so the fixture holds digests only and
tests/test_gpu_pool_sizes.py rebuilds the same inputs from this file: element i of a tensor with seed s is
(((i * 2654435761 + s * 40503) mod 2^32) >> 16) / 4096 - 8 as fp32, then cast to the tensor's dtype.

Shapes: fine tensor (2, 4, 6, 4, C), planar (1, 5, 6, 4, C) (an odd depth), C in {3, 8, 40} (scalar path, one vector, five vectors), fp32 and
bf16; the skip gradient and the up-sampling slice sit at offset 8 of a C + 16 wide tensor (for C = 40 the vector width halves)."""
import ctypes
import hashlib
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pool_2x_digests.json")
CHANNELS = (3, 8, 40)
DTYPES = (torch.float32, torch.bfloat16)
WIDE, OFF = 16, 8                       # the wider tensor has C + 16 channels, the slice starts at channel 8
ADAM_N, ADAM_STEPS = 4099, 3            # 1,024 quads and a 3-element tail
ADAM_KW = dict(lr_t=1e-3, beta1=0.9, beta2=0.999, eps=1e-7, grad_scale=0.5)


def formula(shape, seed, dtype=torch.float32, device="cuda"):
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    v = (((i * 2654435761 + seed * 40503) % (1 << 32)) >> 16).to(torch.float32) / 4096 - 8        # 16 bits: exact in fp32
    return v.reshape(shape).to(dtype).to(device)


def digest(t):
    torch.cuda.synchronize()
    view = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return hashlib.sha256(t.contiguous().view(view).cpu().numpy().tobytes()).hexdigest()


def pool_cases():
    for planar in (False, True):
        for C in CHANNELS:
            for dtype in DTYPES:
                yield planar, C, dtype


def case_key(planar, C, dtype):
    return "%s/C%d/%s" % ("planar" if planar else "3d", C, str(dtype).replace("torch.", ""))


def pool_outputs(api, planar, C, dtype, **kw):
    """{name: tensor} of the six launches of one case.  `api` has maxpool_fwd / maxpool_bwd / upsample_fwd / upsample_bwd with the
    signatures of fmri_hip.ops; `kw` goes to each of them (the tests pass pool=...)"""
    fine = (1, 5, 6, 4, C) if planar else (2, 4, 6, 4, C)
    low = (fine[0], fine[1] if planar else fine[1] // 2, fine[2] // 2, fine[3] // 2, C)
    wide = fine[:-1] + (C + WIDE,)
    x = torch.relu(formula(fine, 1, dtype))                                   # post-ReLU: the zeros tie
    dy, add = formula(low, 2, dtype), formula(wide, 3, dtype)
    new = lambda shape: torch.zeros(shape, dtype=dtype, device="cuda")
    out = {}
    out["maxpool_fwd"] = api.maxpool_fwd(x, new(low), planar=planar, **kw)
    out["maxpool_bwd_add_mask"] = api.maxpool_bwd(x, dy, new(fine), add=add, add_off=OFF, relu_mask=True, planar=planar, **kw)
    out["maxpool_bwd"] = api.maxpool_bwd(x, dy, new(fine), relu_mask=False, planar=planar, **kw)
    out["upsample_fwd"] = api.upsample_fwd(dy, new(wide), y_off=OFF, planar=planar, **kw)          # the whole wide tensor: zeros outside the slice
    out["upsample_bwd_xmask"] = api.upsample_bwd(add, new(low), dy_off=OFF, xmask=dy, planar=planar, **kw)
    out["upsample_bwd"] = api.upsample_bwd(add, new(low), dy_off=OFF, planar=planar, **kw)
    return out


def adam_outputs(adam_step):
    """{name: tensor}: p, m, v after three steps; adam_step has the signature of fmri_hip.ops.adam_step"""
    p, m, v = formula((ADAM_N,), 4), torch.zeros(ADAM_N, device="cuda"), torch.zeros(ADAM_N, device="cuda")
    for step in range(ADAM_STEPS):
        adam_step(p, formula((ADAM_N,), 5 + step), m, v, **ADAM_KW)
    return {"p": p, "m": m, "v": v}


def retired_api(L):
    """the 2x entries of library L behind the signatures of fmri_hip.ops"""
    vp, i32, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    L.fmri_maxpool3d_2x_fwd.argtypes = [vp, vp] + [i32] * 7 + [vp]
    L.fmri_maxpool3d_2x_bwd.argtypes = [vp, vp, vp, i32, i32, vp] + [i32] * 8 + [vp]
    L.fmri_upsample_nearest2x_fwd.argtypes = [vp, vp] + [i32] * 9 + [vp]
    L.fmri_upsample_nearest2x_bwd.argtypes = [vp, i32, i32, vp, vp] + [i32] * 7 + [vp]
    L.fmri_adam_step.argtypes = [vp, vp, vp, vp, ctypes.c_int64] + [f32] * 5 + [vp]
    ptr = lambda t: None if t is None else t.data_ptr()
    dt = lambda t: {torch.float32: 0, torch.bfloat16: 1}[t.dtype]
    stream = lambda: torch.cuda.current_stream().cuda_stream

    def ok(rc):
        assert rc == 0, rc

    def maxpool_fwd(x, y, planar=False):
        N, D, H, W, C = x.shape
        ok(L.fmri_maxpool3d_2x_fwd(ptr(x), ptr(y), N, D, H, W, C, dt(x), int(planar), stream()))
        return y

    def maxpool_bwd(x, dy, dx, add=None, add_off=0, relu_mask=True, planar=False):
        N, D, H, W, C = x.shape
        ok(L.fmri_maxpool3d_2x_bwd(ptr(x), ptr(dy), ptr(add), 0 if add is None else add.shape[-1], add_off, ptr(dx), N, D, H, W, C,
                                   int(relu_mask), dt(x), int(planar), stream()))
        return dx

    def upsample_fwd(x, y, y_off=0, planar=False):
        N, D, H, W, C = x.shape
        ok(L.fmri_upsample_nearest2x_fwd(ptr(x), ptr(y), y.shape[-1], y_off, N, D, H, W, C, dt(x), int(planar), stream()))
        return y

    def upsample_bwd(dy, dx, dy_off=0, xmask=None, planar=False):
        N, D, H, W, C = dx.shape
        ok(L.fmri_upsample_nearest2x_bwd(ptr(dy), dy.shape[-1], dy_off, ptr(xmask), ptr(dx), N, D, H, W, C, dt(dx), int(planar), stream()))
        return dx

    def adam_step(p, g, m, v, lr_t, beta1, beta2, eps, grad_scale):
        ok(L.fmri_adam_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr_t, beta1, beta2, eps, grad_scale, stream()))

    return types.SimpleNamespace(maxpool_fwd=maxpool_fwd, maxpool_bwd=maxpool_bwd, upsample_fwd=upsample_fwd, upsample_bwd=upsample_bwd,
                                 adam_step=adam_step)


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    api = retired_api(ctypes.CDLL(os.environ["FMRI_LIB"]))             # after `import torch`: one HIP runtime in the process
    digests = {}
    for planar, C, dtype in pool_cases():
        for name, t in pool_outputs(api, planar, C, dtype).items():
            digests["%s/%s" % (case_key(planar, C, dtype), name)] = digest(t)
    for name, t in adam_outputs(api.adam_step).items():
        digests["adam/%s" % name] = digest(t)
    with open(sys.argv[1] if len(sys.argv) > 1 else OUT, "w") as f:
        json.dump(digests, f, indent=1, sort_keys=True)
        f.write("\n")
    print("%d digests -> %s" % (len(digests), f.name))


if __name__ == "__main__":
    main()
