"""Agreement of the TTA variants, host side (no GPU): `prediction.tta_agreement(..., device=False)` against the restatement written from
the definitions (tests/tta_agreement_restatement.py), the scores from hand-made counts, the refusals, the entry point in the header, the
binding table and the built library, and the default keyword values leaving `predict_volume`'s keys alone."""
import os
import re
import subprocess

import numpy as np
import pytest

import tta_agreement_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52                                              # one unit in the last place of 1.0


def _volume_stack(kind, K, shape, C, seed):
    nvox = int(np.prod(shape))
    flat = (R.dyadic_stack if kind == "dyadic" else R.smooth_stack)(K, nvox, C, seed)
    return flat.reshape((K,) + shape + ((C,) if C > 1 else ()))


@pytest.mark.parametrize("kind", ["dyadic", "smooth"])
@pytest.mark.parametrize("K,C", [(1, 1), (2, 1), (3, 3), (8, 1), (8, 3), (9, 1), (17, 2)])
def test_host_form_is_the_restatement(kind, K, C):
    from fetal_net.prediction import TTA_MAPS, tta_agreement
    stack = _volume_stack(kind, K, (5, 6, 7), C, 100 * K + C)
    got = tta_agreement(stack, device=False)
    want = R.agreement(stack, 0.5, C)
    assert TTA_MAPS == R.MAPS
    for name in ("median", "mean", "variance", "disagreement"):
        g = getattr(got, name)
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == stack.shape[1:], name
        assert g.tobytes() == want[name].tobytes(), name
    assert float(np.abs(got.entropy - want["entropy"]).max()) <= 4 * ULP
    assert got.counts.dtype == np.int64 and got.counts.shape == (C, 2 * K + 1) and np.array_equal(got.counts, want["counts"])
    assert got.median.tobytes() == np.median(stack, axis=0).tobytes()
    assert got.variance.min() >= 0.0 and 0.0 <= got.entropy.min() and got.entropy.max() <= 1.0
    dice, est, cv = R.scores(want["counts"])
    assert got.variant_dice.shape == (K, C) and got.estimated_dice.shape == (C,) and got.volume_cv.shape == (C,)
    np.testing.assert_allclose(got.variant_dice, dice, rtol=0, atol=2 * ULP)
    np.testing.assert_allclose(got.estimated_dice, est, rtol=0, atol=4 * ULP)
    np.testing.assert_allclose(got.volume_cv, cv, rtol=0, atol=4 * ULP)
    if kind == "dyadic" and K % 2 == 0:
        assert (got.median == 0.5).any()                      # a median exactly on the threshold: not in M


def test_entropy_at_the_ends_and_in_the_middle():
    from fetal_net.prediction import tta_agreement
    stack = np.zeros((4, 1, 1, 5))
    stack[:, 0, 0, 1] = 1.0
    stack[:, 0, 0, 2] = [0.0, 1.0, 0.0, 1.0]
    stack[:, 0, 0, 3] = [-0.5, -0.25, 0.0, 0.0]                 # a mean below 0 is clamped
    stack[:, 0, 0, 4] = [1.5, 1.0, 2.0, 1.0]
    got = tta_agreement(stack, device=False)
    assert got.entropy.reshape(-1).tolist() == [0.0, 0.0, 1.0, 0.0, 0.0]
    assert got.disagreement.reshape(-1).tolist() == [0.0, 0.0, 0.5, 0.0, 0.0]


def test_one_variant_agrees_with_itself():
    from fetal_net.prediction import tta_agreement
    stack = _volume_stack("smooth", 1, (4, 5, 6), 1, 3)
    got = tta_agreement([stack[0]], device=False)
    assert got.median.tobytes() == stack[0].tobytes() == got.mean.tobytes()
    assert not got.variance.any() and not got.disagreement.any()
    assert got.variant_dice.tolist() == [[1.0]] and got.estimated_dice.tolist() == [1.0] and got.volume_cv.tolist() == [0.0]


def test_scores_from_hand_made_counts():
    from fetal_net.prediction import agreement_scores
    #            |M|  |V_0| |V_1|  i_0  i_1
    counts = [[100, 100, 50, 100, 50],                         # variant 0 is the consensus; variant 1 half of it
              [0, 0, 0, 0, 0],                                 # an empty consensus and empty variants: Dice 1
              [0, 10, 30, 0, 0],                               # an empty consensus, non-empty variants: Dice 0
              [40, 0, 0, 0, 0]]
    dice, est, cv = agreement_scores(np.array(counts))
    assert dice.shape == (2, 4)
    assert dice[:, 0].tolist() == [1.0, 2.0 * 50 / 150] and est[0] == (1.0 + 2.0 * 50 / 150) / 2
    assert dice[:, 1].tolist() == [1.0, 1.0] and est[1] == 1.0 and cv[1] == 0.0
    assert dice[:, 2].tolist() == [0.0, 0.0] and est[2] == 0.0
    assert dice[:, 3].tolist() == [0.0, 0.0] and cv[3] == 0.0
    assert cv[0] == np.std([100.0, 50.0]) / 75.0 and cv[2] == 10.0 / 20.0
    one = agreement_scores(np.array([[7, 7, 7]]))              # K = 1
    assert one[0].tolist() == [[1.0]] and one[1].tolist() == [1.0] and one[2].tolist() == [0.0]
    with pytest.raises(ValueError):
        agreement_scores(np.zeros((1, 4), dtype=np.int64))


def test_as_dict_and_requested_maps():
    from fetal_net.prediction import tta_agreement
    stack = _volume_stack("dyadic", 8, (4, 4, 4), 1, 9)
    got = tta_agreement(list(stack), 0.25, maps=("variance",), device=False)
    assert got.mean is None and got.entropy is None and got.disagreement is None and got.threshold == 0.25
    assert set(got.as_dict()) == {"median", "variance", "threshold", "counts", "variant_dice", "estimated_dice", "volume_cv"}
    assert np.array_equal(got.counts, R.agreement(stack, 0.25)["counts"])
    assert got.variance.tobytes() == R.agreement(stack, 0.25)["variance"].tobytes()


def test_refusals():
    from fetal_net.pipeline import Stage
    from fetal_net.prediction import tta_agreement
    with pytest.raises(ValueError):
        tta_agreement([], device=False)
    with pytest.raises(ValueError):
        tta_agreement(np.zeros((0, 4, 4, 4)), device=False)
    with pytest.raises(ValueError):
        tta_agreement(np.zeros((65, 2, 2, 2)), device=False)
    with pytest.raises(ValueError):
        tta_agreement(np.zeros((2, 2, 2, 2, 17)), device=False)
    with pytest.raises(ValueError):
        tta_agreement(np.zeros((2, 4, 4, 4), dtype=np.float32), device=False)
    with pytest.raises(ValueError):
        tta_agreement(np.zeros((2, 4, 4)), device=False)
    with pytest.raises(ValueError):
        tta_agreement(np.zeros((2, 4, 4, 4)), maps=("median",), device=False)
    tta_agreement(np.zeros((64, 2, 2, 2, 16)), device=False)
    stage = Stage(_NeighbourModel((8, 8, 8)), {"patch_shape": [8, 8], "patch_depth": 8}, augment=None, device=False)
    with pytest.raises(ValueError):
        stage.infer(np.zeros((8, 8, 8)), agreement=True)


PARAMETERS = ("const double* stack, int K, int64_t nvox, int C, double threshold, double* median, double* mean, double* variance, "
              "double* entropy, double* disagreement, uint64_t* counts, fmri_stream_t stream")


def test_entry_point_in_header_binding_table_and_library():
    import ctypes
    from fmri_hip._lib import LIB_PATH, SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "fmri_hip.h")).read()
    m = re.search(r"^int fmri_tta_agreement_f64\(([^;]*)\);", header, re.M)
    assert m and " ".join(m.group(1).split()) == PARAMETERS
    p, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
    assert SIGNATURES["fmri_tta_agreement_f64"] == [p, i32, i64, i32, f64, p, p, p, p, p, p, p]
    if not os.path.exists(LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(lib(), "fmri_tta_agreement_f64")
    out = subprocess.check_output(["nm", "-D", "--defined-only", LIB_PATH]).decode()
    assert re.search(r"\bT fmri_tta_agreement_f64\b", out)


class _NeighbourModel:
    """predict(x) = sigmoid of a voxel and its neighbour along the last axis: it does not commute with the flips, so the eight variants
    differ (tests/test_host_pipeline.py's point-wise model gives eight equal ones)"""

    def __init__(self, patch):
        self.output_shape = (None, 1) + tuple(patch)

    def predict(self, x):
        x = np.asarray(x, dtype=np.float64)
        return 1.0 / (1.0 + np.exp(-3.0 * (0.5 * x + 0.5 * np.roll(x, 1, axis=-1))))


def test_defaults_keep_the_keys_and_the_flag_adds_agreement():
    from fetal_net.pipeline import Stage, predict_volume
    from fetal_net.prediction import TTAAgreement, tta_agreement
    rs = np.random.RandomState(4)
    vol = rs.randn(20, 24, 12)
    patch = (8, 8, 8)
    cfg = {"patch_shape": list(patch[:2]), "patch_depth": patch[2]}
    m = _NeighbourModel(patch)
    plain = predict_volume(vol, m, cfg, overlap_factor=0.5, augment="flip", device=False)
    assert set(plain) == {"data", "prediction"}
    two = predict_volume(vol, m, cfg, overlap_factor=0.5, augment="flip", model2=m, config2=cfg, augment2="flip", device=False)
    assert set(two) == {"data", "prediction", "mask", "prediction_roi"}
    out = predict_volume(vol, m, cfg, overlap_factor=0.5, augment="flip", model2=m, config2=cfg, augment2="flip", device=False,
                         return_agreement=True)
    assert set(out) == {"data", "prediction", "mask", "prediction_roi", "agreement", "agreement_roi"}
    for key in two:
        assert np.asarray(out[key]).tobytes() == np.asarray(two[key]).tobytes(), key
    assert out["prediction"].tobytes() == plain["prediction"].tobytes()
    for key in ("agreement", "agreement_roi"):
        a = out[key]
        assert isinstance(a, TTAAgreement) and a.counts.shape == (1, 17)
        for name in ("median", "mean", "variance", "entropy", "disagreement"):
            assert getattr(a, name).shape == vol.shape, (key, name)
        assert 0.0 <= a.estimated_dice[0] <= 1.0
    a = out["agreement"]
    assert a.median.tobytes() == out["prediction"].tobytes() and a.variance.max() > 0.0
    # the stage alone: the agreement of the very stack it returns; counts on the grid the model saw (the border included)
    stage = Stage(m, cfg, augment="flip", overlap=0.5, device=False, threshold=0.6)
    kept, agreed = stage.infer(vol, keep_variants=True, agreement=True)
    want = R.agreement(kept, 0.6)
    assert kept.shape == (8,) + vol.shape and agreed.threshold == 0.6
    assert np.array_equal(agreed.counts, want["counts"]) and agreed.variance.tobytes() == want["variance"].tobytes()
    assert agreed.counts[0, 0] == int((agreed.median > 0.6).sum()) > 0
    pred, again = stage.infer(vol, agreement=True)
    assert pred.tobytes() == stage.infer(vol).tobytes() == again.median.tobytes()
    assert np.array_equal(again.counts, agreed.counts)
    assert tta_agreement(kept, 0.6, device=False).median.tobytes() == pred.tobytes()
