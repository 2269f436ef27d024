"""Helpers the training-step suites (tests/test_*_step_gpu.py) share: the bitwise-reproducible step, a student with the feature streams'
dropout out of the way, and the launch census of a callable."""
import ctypes as C

import pytest
import torch

from tests.test_model_gpu import build_model


@pytest.fixture
def deterministic_embed(monkeypatch):
    """The atomic-free embedding-table gradient: the whole step is bitwise reproducible (tests/test_model_gpu.py)."""
    from mtn_amd import lib
    monkeypatch.setenv("MTN_EMBED_DETERMINISTIC", "1")
    lib.reload_env()
    yield
    monkeypatch.delenv("MTN_EMBED_DETERMINISTIC")
    lib.reload_env()


def _student(c, dtype, dev, dropout):
    model = build_model(c, dtype, dev, dropout=dropout, attn_dropout=dropout).train()
    for mod in model.modules():                 # the feature streams' dropout is PyTorch's (its own RNG): keep it out
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    model.prepare()
    if model._seed is not None:
        model._seed.fill_(4242)
    return model


def _census(fn):
    """[(kernel variant, workgroups, problems, first problem's M x N x K)] of every GEMM launch of fn(), and the fused-group counters."""
    from mtn_amd import lib as L
    lib = L.load()
    f0 = L.fused_counters()
    lib.mtn_census_begin()
    fn()
    torch.cuda.synchronize()
    n = lib.mtn_census_end()
    rows = []
    for i in range(n):
        info = L.CensusLaunch()
        L.check(lib.mtn_census_info(i, C.byref(info)))
        rows.append((lib.mtn_census_variant_name(info.variant).decode(), info.workgroups, info.count, (info.M[0], info.N[0], info.K[0])))
    return rows, tuple(a - b for a, b in zip(L.fused_counters(), f0))
