"""Host side of FMRI_DETERMINISTIC=1 (no GPU): the two entry points of the ordered normalisation statistics in the header, the binding
table and the library; their host-only arithmetic and argument checks; the chain's rule that both engines run in one mode."""
import os
import types

import pytest

from conftest import ROOT

NAMES = ("fmri_set_deterministic_scratch", "fmri_norm_det_workspace_bytes")


def test_scratch_entry_points_are_declared_bound_and_exported():
    from fmri_hip._lib import SIGNATURES, lib
    header = open(os.path.join(ROOT, "include", "fmri_hip.h")).read()
    for n in NAMES:
        assert n + "(" in header and n in SIGNATURES and hasattr(lib(), n), n


def test_workspace_bytes_counts_one_row_per_reduction_workgroup():
    from fmri_hip._lib import lib
    L = lib()
    N, V, C = 2, 16 * 16 * 16, 8
    for per in (0, 1):
        b = L.fmri_norm_det_workspace_bytes(N, V, C, per)
        assert b > 0 and b % (16 * C * N) == 0                    # rows = N x workgroups per sample, {sum, sum2} doubles per channel
        assert b // (16 * C * N) > 1                              # the op-level GPU test's shape: several workgroups per (group, channel)
    # the cap of 4096 voxels per workgroup: a 128^3 sample gives 512 rows
    assert L.fmri_norm_det_workspace_bytes(1, 128 ** 3, 16, 1) == 512 * 16 * 16
    assert L.fmri_norm_det_workspace_bytes(0, V, C, 0) == 0 and L.fmri_norm_det_workspace_bytes(N, V, 0, 0) == 0


def test_scratch_registration_checks_its_arguments():
    from fmri_hip._lib import lib
    L = lib()
    assert L.fmri_set_deterministic_scratch(0, 0) == 0
    assert L.fmri_set_deterministic_scratch(0, 64) == -1         # a size without a pointer
    assert L.fmri_set_deterministic_scratch(4096, 0) == -1       # a pointer without a size
    assert L.fmri_set_deterministic_scratch(4100, 64) == -1      # not 8-byte aligned
    assert L.fmri_set_deterministic_scratch(0, 0) == 0


def test_switch_is_read_by_the_shared_engine_base(monkeypatch):
    from fmri_hip.engine_base import read_switches
    monkeypatch.delenv("FMRI_DETERMINISTIC", raising=False)
    assert read_switches(DETERMINISTIC=False)["DETERMINISTIC"] is False
    monkeypatch.setenv("FMRI_DETERMINISTIC", "1")
    assert read_switches(DETERMINISTIC=False)["DETERMINISTIC"] is True
    import inspect
    from fmri_hip import engine_base, graph_engine
    assert "DETERMINISTIC=False" in inspect.getsource(engine_base.EngineBase.__init__)
    assert "_det_register" in inspect.getsource(graph_engine.LayerGraphEngine)


def test_chain_refuses_engines_in_different_modes():
    from fmri_hip.chain_engine import ChainEngine
    norm = types.SimpleNamespace(linear=True, deterministic=True)
    for seg in (types.SimpleNamespace(input_grad=True, training=True, deterministic=False, frozen=True),
                types.SimpleNamespace(input_grad=True, training=True, deterministic=True, frozen=False)):
        with pytest.raises(ValueError, match="FMRI_DETERMINISTIC"):
            ChainEngine(norm, seg)
