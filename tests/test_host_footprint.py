"""The footprint checker itself (tests/footprint.py), on the CPU: fake "ops" written in torch with one deliberate defect each must make
audit() raise and name the tensor; a correct op passes at both placements."""
import pytest
import torch

import footprint as fp
from footprint import Arena, Plain, audit

N = 37


def _x():
    return torch.arange(1, N + 1, dtype=torch.float32) * 0.25


def _peek(t, delta, n=1):
    """n elements of t's storage starting `delta` elements from its first one (what a kernel's stray pointer sees)"""
    return torch.as_strided(t, (n,), (1,), t.storage_offset() + delta)


def good(alloc, offset16=False):
    x = alloc.input(_x(), offset16=offset16, name="x")
    y = alloc.output((N,), torch.float32, offset16=offset16, name="y")
    acc = alloc.accumulate(torch.ones(N), offset16=offset16, name="acc")
    ws = alloc.workspace(N * 8, zero=True, dtype=torch.float64, name="ws")
    scratch = alloc.workspace(N * 4, dtype=torch.float32, name="scratch")
    wide = alloc.output((N, 6), torch.float32, name="wide")
    alloc.slot(wide[:, 2:5], wide)
    ws += x.double()
    scratch.copy_(x)
    y.copy_(scratch * 2 + ws.float())
    acc += x
    wide[:, 2:5] = x[:, None]
    ws.zero_()
    return {"y": y, "acc": acc, "wide": wide[:, 2:5], "sum": x.sum().reshape(1)}


def test_a_correct_op_passes_at_both_placements():
    audit(good, device="cpu")
    audit(lambda a: good(a, offset16=True), device="cpu")


def test_placements_and_guards():
    a = Arena("cpu", 4 << 20)
    t0 = a.take((5, 7), torch.float32, "output")
    t1 = a.take((3,), torch.float32, "accumulate", fill=torch.zeros(3), offset16=True)
    t2 = a.take((2, 40000), torch.bfloat16, "output")                 # one outermost slice = 80000 bytes > 64 KiB
    w = a.workspace(24)
    t3 = a.input(torch.zeros(9, dtype=torch.float64), offset16=True)
    assert t0.data_ptr() % 256 == 0 and t2.data_ptr() % 256 == 0 and w.data_ptr() % 256 == 0
    assert t1.data_ptr() % 256 == 16 and t3.data_ptr() % 256 == 16
    assert t0.is_contiguous() and t2.is_contiguous() and w.numel() == 24 and w.dtype == torch.uint8
    for i in range(len(a.spans)):
        assert a.guard_before(i) >= 64 * 1024 and a.guard_behind(i) >= 64 * 1024, (i, a.spans[i])
    assert a.guard_before(2) >= 80000 and a.guard_behind(2) >= 80000
    # the fill is NaN / 255 / -1
    assert bool(torch.isnan(t0).all()) and bool(torch.isnan(t2).all()) and int(w[0]) == 255
    assert int(a.buf[a.base:a.base + 4].view(torch.int32)[0]) == -1 and bool(torch.isnan(a.buf[a.base:a.base + 8].view(torch.float64)).all())
    a.check_guards()
    with pytest.raises(MemoryError):
        Arena("cpu", 100 * 1024).take((4,), torch.float32, "output")


def _defect(kind):
    def run(alloc):
        x = alloc.input(_x(), name="x_in")
        y = alloc.output((N,), torch.float32, name="y_out")
        ws = alloc.workspace(N * 4, dtype=torch.float32, name="scratch_ws")
        zws = alloc.workspace(N * 8, zero=True, dtype=torch.float64, name="zero_ws")
        wide = alloc.output((N, 6), torch.float32, name="wide_out")
        alloc.slot(wide[:, 2:5], wide)
        ws.copy_(x)
        y.copy_(ws * 2)
        wide[:, 2:5] = x[:, None]
        total = x.sum()
        if kind == "past_end":
            _peek(y, N).fill_(1.0)
        elif kind == "before_start":
            _peek(y, -1).fill_(1.0)
        elif kind == "behind_workspace":
            _peek(ws, N).fill_(0.0)
        elif kind == "unwritten":
            y[N - 1] = float("nan")
        elif kind == "input_modified":
            x[3] += 1.0
            x[3] -= 0.5
        elif kind == "sentinel":
            wide[N // 2, 5] = 2.0
        elif kind == "workspace_nonzero":
            zws[N - 1] = 1e-300
        elif kind == "reads_behind_input":
            total = _peek(x, 0, N + 1).sum()            # one element too many: 0 of slack on a plain tensor, NaN in the arena
        else:
            assert kind == "none"
        return {"y": y, "wide": wide[:, 2:5], "total": total.reshape(1)}
    return run


DEFECTS = [("past_end", "BEHIND y_out"), ("before_start", "IN FRONT OF y_out"), ("behind_workspace", "BEHIND scratch_ws"),
           ("unwritten", "y_out: output not fully written"), ("input_modified", "x_in: input modified"),
           ("sentinel", "wide_out: sentinel column 5"), ("workspace_nonzero", "zero_ws: zero-on-exit workspace left nonzero"),
           ("reads_behind_input", "total")]


@pytest.mark.parametrize("kind,names", DEFECTS, ids=[d[0] for d in DEFECTS])
def test_each_defect_is_caught_and_names_the_tensor(kind, names):
    audit(_defect("none"), device="cpu")                 # the same op without the defect passes
    with pytest.raises(AssertionError) as e:
        audit(_defect(kind), device="cpu")
    assert names in str(e.value), str(e.value)


def test_guard_report_gives_the_side_and_the_distance():
    a = Arena("cpu", 1 << 20)
    t = a.take((8,), torch.float32, "output", name="t")
    u = a.take((8,), torch.float32, "output", name="u")
    _peek(t, 8 + 2).fill_(0.0)                           # bytes 8..11 past t's end
    with pytest.raises(AssertionError, match=r"4 bytes BEHIND t, the nearest 9 bytes past its end \(the farthest 12\)"):
        a.check_guards()
    _peek(t, 8 + 2).view(torch.int32).fill_(-1)
    _peek(u, -4).fill_(0.0)                              # bytes 16..13 before u's start
    with pytest.raises(AssertionError, match=r"4 bytes IN FRONT OF u, the nearest 13 bytes before its start \(the farthest 16\)"):
        a.check_guards()


def test_an_integer_output_left_unwritten_differs_between_the_runs():
    def run(alloc, skip):
        lab = alloc.output((N,), torch.uint8, name="labels")
        lab[:N - skip] = 3
        return {"labels": lab}
    audit(lambda a: run(a, 0), device="cpu")
    with pytest.raises(AssertionError, match="labels"):
        audit(lambda a: run(a, 1), device="cpu")


def test_plain_allocator_hands_out_separate_tensors_and_sizes_the_arena():
    p = Plain("cpu")
    a = p.take((5,), torch.float32, "output")
    b = p.workspace(40)
    assert a.untyped_storage().data_ptr() != b.untyped_storage().data_ptr()
    ar = Arena("cpu", p.required_bytes())
    ar.take((5,), torch.float32, "output")
    ar.workspace(40)
    assert fp.guard_bytes((5,), torch.float32) == 64 * 1024
