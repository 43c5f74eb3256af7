"""The launch schedule of UNetEngine, recorded on the CPU.

An engine built with device="cpu" runs whole steps once every launcher of fmri_hip.ops is replaced by a recorder: the host-side queries
(*_ok, *_bytes, *_doubles, is_overlap_loss, loss_value_from_sums, dt) stay real and answer from the library without a device, and
fwd_cu_count() falls back to the MI355X's 256, so the engine plans the routes it plans on the GPU.  What is recorded, one line per event:
  * every call of a function defined in fmri_hip.ops that is not a query: its name and its bound arguments in the order of its
    signature, defaults applied;
  * every aten op with a mutable schema (copy_, add_, zero_, index_put_, ...): the torch-side arithmetic of the fold / onetap / d2s
    routes and the gradient zeroing belong to the schedule;
  * begin / grad_ready(name) / finish of a recording data-parallel context;
  * the route plan of every buffer set the case switches to.
A tensor is written T<k>+<storage offset><shape><strides><dtype>, k numbering the storages in order of first appearance: the text depends
on neither attribute names nor addresses, and is the same from process to process.  The recorder keeps every tensor it has seen, so the
address of a freed temporary cannot come back as another tensor.

tests/golden/engine_schedule.json holds the lines of every case below as the engine issued them before its decoder routes were gathered
into classes (tests/golden/make_engine_schedule_fixture.py); tests/test_host_engine_schedule.py compares.  The file keeps every distinct
line and every distinct tensor layout once (`pack`), so that it stays small enough to read; `unpack` gives the full lines back.
"""
import contextlib
import inspect
import json
import os
import re

import torch
from torch.utils._python_dispatch import TorchDispatchMode

QUERIES = ("dt", "is_overlap_loss", "loss_value_from_sums")
QUERY_SUFFIXES = ("_ok", "_bytes", "_doubles")
DTYPES = {torch.bfloat16: "bf16", torch.float32: "f32", torch.float64: "f64", torch.int64: "i64", torch.uint8: "u8"}
RESULT_ARGS = ("y", "dst", "dx", "out")          # the argument a launcher hands back, where the engine uses the result


class Recorder(object):
    def __init__(self):
        self.lines, self._seen, self._storages = [], [], {}

    def enc(self, v):
        if isinstance(v, torch.Tensor):
            self._seen.append(v)
            k = self._storages.setdefault(v.untyped_storage()._cdata, len(self._storages))
            dims = lambda d: "[%s]" % ",".join(str(int(e)) for e in d)
            return "T%d+%d%s%s%s" % (k, v.storage_offset(), dims(v.shape), dims(v.stride()), DTYPES.get(v.dtype, str(v.dtype)[6:]))
        if isinstance(v, (list, tuple)):
            return "(" + ",".join(self.enc(e) for e in v) + ")"
        if isinstance(v, dict):
            return "{" + ",".join("%s:%s" % (k, self.enc(v[k])) for k in sorted(v)) + "}"
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        if isinstance(v, (torch.dtype, torch.device, torch.memory_format, torch.layout)):
            return str(v)
        return "<%s>" % type(v).__name__

    def add(self, name, args):
        self.lines.append("%s(%s)" % (name, ", ".join(self.enc(a) for _, a in args)))


LAYOUT = re.compile(r"(T\d+)(\+\d+\[[0-9,]*\]\[[0-9,]*\][a-z0-9]+)")


def pack(cases):
    """{case: lines} -> {"layouts": the distinct +<offset><shape><strides><dtype> texts, "lines": the distinct lines with @<n> for
    layouts[n], "cases": {case: indices into lines}}"""
    layouts, lines = {}, {}
    assert not any("@" in line for v in cases.values() for line in v)
    short = lambda line: LAYOUT.sub(lambda m: "%s@%d" % (m.group(1), layouts.setdefault(m.group(2), len(layouts))), line)
    out = {case: [lines.setdefault(short(line), len(lines)) for line in v] for case, v in cases.items()}
    return dict(layouts=list(layouts), lines=list(lines), cases=out)


def unpack(fixture):
    full = [re.sub(r"@(\d+)", lambda m: fixture["layouts"][int(m.group(1))], line) for line in fixture["lines"]]
    return {case: [full[i] for i in idx] for case, idx in fixture["cases"].items()}


class _AtenMode(TorchDispatchMode):
    def __init__(self, rec):
        super().__init__()
        self.rec = rec

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        if func._schema.is_mutable:
            self.rec.lines.append("aten.%s(%s)" % (str(func).replace("aten.", ""), ", ".join(
                [self.rec.enc(a) for a in args] + ["%s=%s" % (k, self.rec.enc(kwargs[k])) for k in sorted(kwargs)])))
        return func(*args, **kwargs)


class RecordingDist(object):
    """a one-rank data-parallel context with per-rank losses that logs what the engine tells it"""
    world, grad_scale, global_dice = 1, 1.0, False

    def __init__(self, rec):
        self.rec = rec

    def begin(self):
        self.rec.lines.append("dist.begin()")

    def grad_ready(self, eng, name):
        self.rec.lines.append("dist.grad_ready(%s)" % name)

    def finish(self, eng):
        self.rec.lines.append("dist.finish()")


def launchers(ops):
    """name -> function for every public function defined in fmri_hip.ops that is not a host-side query"""
    out = {}
    for name, f in vars(ops).items():
        if (inspect.isfunction(f) and f.__module__ == ops.__name__ and not name.startswith("_") and name not in QUERIES
                and not name.endswith(QUERY_SUFFIXES)):
            out[name] = f
    return out


def _wrapper(rec, name, f):
    sig = inspect.signature(f)

    def call(*a, **kw):
        b = sig.bind(*a, **kw)
        b.apply_defaults()
        rec.add(name, list(b.arguments.items()))
        if name == "pack_table":
            return torch.zeros((len(b.arguments["entries"]), 10), dtype=torch.int64), len(b.arguments["entries"])
        for r in RESULT_ARGS:
            if r in b.arguments:
                return b.arguments[r]
        return None
    return call


@contextlib.contextmanager
def recording(rec):
    """fmri_hip.ops' launchers replaced by recorders and the mutable aten ops logged, for the length of the block"""
    from fmri_hip import ops
    real = launchers(ops)
    for name, f in real.items():
        setattr(ops, name, _wrapper(rec, name, f))
    try:
        with _AtenMode(rec):
            yield rec
    finally:
        for name, f in real.items():
            setattr(ops, name, f)


# ---------------------------------------------------------------------------------------------------------------------- cases
# Each case is the smallest shape at which the named route or tail is planned.  plan: UNetPlan arguments; env: the FMRI_* switches of the
# case (Python-side ones only: the C-side ones are read once per process); up: route["up"] per buffer set, deepest decoder level first;
# run: "train" (two train_steps per entry of `batches`, on one engine), "predict" or "frozen".
_UP3D = dict(in_channels=1, spatial=(16, 32, 32), depth=3, n_base_filters=32)
_D2 = dict(in_channels=1, spatial=(16, 32, 32), depth=2, n_base_filters=32)
_2D = dict(in_channels=5, spatial=(64, 64), depth=3, n_base_filters=32, ndim=2)
_NT = dict(in_channels=1, spatial=(32, 64, 64), depth=3, n_base_filters=32)
BF16, F32 = "bfloat16", "float32"


def _case(plan, batches=(1,), dtype=BF16, env=None, up=None, run="train", steps=2, **engine):
    return dict(plan=plan, batches=list(batches), dtype=dtype, env=env or {}, up=up, run=run, steps=steps, engine=engine)


CASES = {
    "up3d": _case(_UP3D, up=[["upsample", "upcat"]]),
    "up3d_fp32": _case(dict(_UP3D, n_base_filters=8), dtype=F32, up=[["upsample", "upsample"]]),
    "up3d_upcat0": _case(_UP3D, env={"FMRI_UPCAT": "0"}, up=[["upsample", "upsample"]]),
    "fold": _case(dict(_UP3D, deconvolution=True), up=[["deconv", "fold"]]),
    "onetap": _case(dict(_UP3D, deconvolution=True), env={"FMRI_DECONV_FOLD": "0"}, up=[["deconv", "onetap"]]),
    "onetap_norm": _case(dict(_D2, norm="instance", deconvolution=True), batches=(2,), up=[["onetap"]], input_grad=True),
    "deconv_fp32": _case(dict(_D2, n_base_filters=8, deconvolution=True), dtype=F32, up=[["deconv"]]),
    "bn": _case(dict(_UP3D, norm="batch"), batches=(2,), up=[["upsample", "upcat"]]),
    "ntails_batch": _case(dict(_NT, norm="batch"), batches=(2,), env={"FMRI_NORM_FUSE": "3", "FMRI_NORM_FUSE_MAXLEVEL": "9"}),
    "ntails_instance": _case(dict(_NT, norm="instance"), batches=(2,), env={"FMRI_NORM_FUSE": "3", "FMRI_NORM_FUSE_MAXLEVEL": "9"}),
    "2d": _case(_2D, batches=(8,), up=[["upcat", "upcat"]]),
    "2d_odd": _case(_2D, batches=(6,), up=[["upsample", "upsample"]]),
    "2d_d2s_sets": _case(dict(_2D, deconvolution=True), batches=(8, 6, 8), steps=1, up=[["d2s", "d2s"], ["deconv", "deconv"], ["d2s", "d2s"]]),
    "dist": _case(_UP3D, up=[["upsample", "upcat"]], dist=True),
    "infer": _case(_UP3D, run="predict", up=[["upsample", "upcat"]], training=False),
    "frozen": _case(dict(_D2, norm="batch"), batches=(2,), run="frozen", input_grad=True),
}


def record(case):
    """the lines of one case; the FMRI_* environment is the case's own while it runs"""
    from fmri_hip.engine import UNetEngine, UNetPlan
    c = CASES[case]
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("FMRI_")}
    os.environ.update(c["env"])
    rec = Recorder()
    try:
        with recording(rec):
            kw = dict(c["engine"])
            if kw.pop("dist", False):
                kw["dist_ctx"] = RecordingDist(rec)
            dtype = getattr(torch, c["dtype"])
            plan = UNetPlan(**c["plan"])
            eng = UNetEngine(plan, c["batches"][0], dtype=dtype, device="cpu", seed=7, **kw)
            for i, N in enumerate(c["batches"]):
                eng.set_batch(N)
                rec.lines.append("route N=%d %s" % (N, json.dumps(eng.route, sort_keys=True)))
                if c["up"] is not None:
                    assert list(eng.route["up"].values()) == c["up"][i], (case, N, eng.route["up"])
                x = torch.zeros(eng._dims(0) + (plan.in_channels,), dtype=dtype)
                y = torch.zeros(x.numel() // plan.in_channels * plan.n_labels, dtype=torch.uint8)
                if c["run"] == "predict":
                    eng.predict(x)
                elif c["run"] == "frozen":
                    eng.forward(x, update_moving=False)
                    eng.loss_forward(y)
                    eng.backward(y, params=False)
                else:
                    for _ in range(c["steps"]):
                        eng.train_step(x, y, 1e-4)
            if case.startswith("ntails"):
                assert sum(eng.route["stats"].values()) + sum(eng.route["dz"].values()) >= 3, (case, eng.route)
        return rec.lines
    finally:
        for k in c["env"]:
            os.environ.pop(k, None)
        os.environ.update(saved)
