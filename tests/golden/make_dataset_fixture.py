#!/usr/bin/env python3
"""Generate dataset_golden.npz: what the REFERENCE's own data-file code makes of three small subjects.

Runs ONLY where a checkout of the reference project is:
    python tests/golden/make_dataset_fixture.py <reference checkout>
It imports the reference's fetal_net/data.py, normalize.py and preprocess.py where they lie, under stubs for what is not installed
(nibabel / nilearn / PyTables): `read_img` is backed by this package's NIfTI reader, and the VLArrays are a list with a `.shape`.
`write_image_data_to_file` (data.py:20-32) and `normalize_data_storage` / `normalize_data_storage_each` (normalize.py:72-92) then run
as they are, on three ragged subjects, for scale in {None, (0.5, 0.5, 1)} x preproc in {None, laplace_norm} x {without, with} mask file.

Output (committed; arrays only):
    vol_<i>, truth_<i>, maskin_<i>                          the inputs (float64, uint8, float64), as written to the NIfTI files
    <case>_data_<i>, <case>_truth_<i>, <case>_mask_<i>      the storages after write_image_data_to_file
    <case>_all_<i>, <case>_mean, <case>_std                 after normalize_data_storage
    <case>_each_<i>                                         after normalize_data_storage_each
with <case> = s<0|1>p<0|1>m<0|1>.  A mask file changes nothing but the mask storage (asserted here), so the m1 cases store only
their truth and mask arrays.
"""
import importlib.util
import os
import shutil
import sys
import tempfile
import types

import numpy as np

np.float = float                     # reference data.py:36 uses the removed alias

REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.environ.get("FETAL_REFERENCE", "")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "..", "fetal-mri-segmentation_amd"))
from fetal_net.utils.nifti import load_nifti, save_nifti  # noqa: E402

SHAPES = [(12, 10, 6), (9, 11, 7), (10, 10, 5)]
SCALES = [None, (0.5, 0.5, 1)]
PREPROCS = [None, "laplace_norm"]


class _Image(object):
    def __init__(self, path):
        self._path = path

    def get_data(self):
        return load_nifti(self._path)


class _Storage(list):
    """what the reference uses of a VLArray: append, [i], [i] = value, .shape[0]"""

    @property
    def shape(self):
        return (len(self),)


def load_reference_modules():
    ours = [k for k in sys.modules if k == "fetal_net" or k.startswith("fetal_net.")]
    for k in ours:
        del sys.modules[k]
    pkg = types.ModuleType("fetal_net")
    pkg.__path__ = [os.path.join(REF, "fetal_net")]
    sys.modules["fetal_net"] = pkg
    up = types.ModuleType("fetal_net.utils")
    up.__path__ = []
    up.crop_img = up.crop_img_to = up.read_image = None
    sys.modules["fetal_net.utils"] = up
    uu = types.ModuleType("fetal_net.utils.utils")
    uu.read_img = _Image
    uu.resize = uu.read_image_files = None
    sys.modules["fetal_net.utils.utils"] = uu
    for name, attrs in (("tables", ()), ("nilearn", ()), ("nilearn.image", ("new_img_like",))):
        m = types.ModuleType(name)
        for a in attrs:
            setattr(m, a, None)
        sys.modules[name] = m
    out = {}
    for name in ("normalize", "preprocess", "data"):
        spec = importlib.util.spec_from_file_location("fetal_net." + name, os.path.join(REF, "fetal_net", name + ".py"))
        m = importlib.util.module_from_spec(spec)
        sys.modules["fetal_net." + name] = m
        spec.loader.exec_module(m)
        out[name] = m
    return out


def main():
    if not os.path.isdir(os.path.join(REF, "fetal_net")):
        sys.exit("usage: make_dataset_fixture.py <reference checkout>")
    rs = np.random.RandomState(11)
    arrays, files = {}, []
    tmp = tempfile.mkdtemp()
    for i, sh in enumerate(SHAPES):
        vol = rs.randn(*sh) * 100 + 300
        truth = (rs.rand(*sh) > 0.6).astype(np.uint8)
        mask = rs.rand(*sh) * 5
        arrays["vol_%d" % i], arrays["truth_%d" % i], arrays["maskin_%d" % i] = vol, truth, mask
        names = [os.path.join(tmp, "s%d_%s.nii.gz" % (i, k)) for k in ("volume", "truth", "mask")]
        for a, p in zip((vol, truth, mask), names):
            save_nifti(a, p)
            back = load_nifti(p)
            assert back.dtype == a.dtype and np.array_equal(back, a)
        files.append(tuple(names))
    R = load_reference_modules()
    D, N, P = R["data"], R["normalize"], R["preprocess"]
    for si, scale in enumerate(SCALES):
        for pi, pre in enumerate(PREPROCS):
            for mi in (0, 1):
                case = "s%dp%dm%d" % (si, pi, mi)
                data, truth, mask = _Storage(), _Storage(), _Storage()
                D.write_image_data_to_file([f if mi else f[:2] for f in files], data, truth, mask, truth_dtype=np.uint8, scale=scale,
                                           preproc=getattr(P, pre) if pre else None)
                assert len(mask) == (len(files) if mi else 0)
                all_, each = _Storage(a.copy(order="K") for a in data), _Storage(a.copy(order="K") for a in data)     # memory order kept, as a pickled row keeps it
                _, mean, std = N.normalize_data_storage(all_)
                _, m2, s2 = N.normalize_data_storage_each(each)
                assert m2 is None and s2 is None
                got = {"mean": np.asarray(mean), "std": np.asarray(std)}
                for i in range(len(files)):
                    assert data[i].dtype == np.float64 and truth[i].dtype == np.uint8
                    got["data_%d" % i], got["truth_%d" % i], got["all_%d" % i], got["each_%d" % i] = data[i], truth[i], all_[i], each[i]
                    if mi:
                        got["mask_%d" % i] = mask[i]
                if mi:
                    base = "s%dp%dm0_" % (si, pi)
                    for k, v in got.items():
                        if not k.startswith(("mask_", "truth_")):
                            assert np.array_equal(arrays[base + k], v)
                    got = {k: v for k, v in got.items() if k.startswith(("mask_", "truth_"))}
                for k, v in got.items():
                    arrays["%s_%s" % (case, k)] = v
    shutil.rmtree(tmp)
    out = os.path.join(HERE, "dataset_golden.npz")
    np.savez_compressed(out, **arrays)
    print("dataset_golden.npz:", os.path.getsize(out), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
