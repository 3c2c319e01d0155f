"""tests/rescaler_check.py without a GPU: the emulation of the kernels' arithmetic stays below a quarter of every bound, the
one-pass E[x^2] - mean^2 formula exceeds the std bound on the sensitivity column (so the bound is sharp enough to catch the wrong
algorithm), the host logic of training.init_hypernet_state, and the C ABI surface and refusals of csrc/train_init.hip."""
import ctypes as C
import os
import re

import pytest
import torch

from tests import rescaler_check as rk
from zett_amd import _lib, synth, training
from zett_amd.config import ZettHypernetConfig
from zett_amd.hypernet import EMBED_INIT_RANGE, ZettHypernet

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zett_op_col_moments_workspace_bytes", "zett_op_col_moments", "zett_op_rescaler_fit")
F64 = torch.float64


def _ratio(got, ref, bnd):
    err = (got.to(F64) - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300)).max())


def _quarter(what, x, calls=None):
    """the emulation of the moments of x (fed as `calls`) and of both fits against the float64 references: largest err / bound"""
    ref = rk.moments_ref(x)
    bnd = rk.moments_bound(x, ref)
    emu = rk.emulate_moments(calls or [x])
    assert torch.equal(emu["count"], ref["count"])
    worst = max(_ratio(emu[k], ref[k], bnd[k]) for k in ("mean", "m2", "std"))
    w64, b64 = rk.scale_to_ref(x, target_stds=torch.full((x.shape[1],), EMBED_INIT_RANGE, dtype=F64), target_means=torch.zeros(x.shape[1], dtype=F64))
    bw, bb = rk.fit_bound(ref, bnd, target_std=EMBED_INIT_RANGE, target_mean=0.0)
    w, b = rk.emulate_fit(emu, target_std=EMBED_INIT_RANGE, target_mean=0.0)
    worst = max(worst, _ratio(w, w64[0], bw), _ratio(b, b64[0], bb))
    # against a target of the same width: the matrix itself, rows reversed and shifted (another mean, the same std)
    t = (x.to(F64).flip(0) * 0.5 + 0.25).to(x.dtype)
    tref = rk.moments_ref(t)
    tbnd = rk.moments_bound(t, tref)
    w64, b64 = rk.scale_to_ref(x, t)
    bw, bb = rk.fit_bound(ref, bnd, tref, tbnd)
    w, b = rk.emulate_fit(emu, rk.emulate_moments([t]))
    worst = max(worst, _ratio(w, w64[0], bw), _ratio(b, b64[0], bb))
    assert worst <= 0.25, (what, worst)
    return worst


@pytest.mark.parametrize("case", rk.pairwise_cases(), ids=lambda c: "x".join(map(str, c)))
def test_emulation_within_a_quarter_of_every_bound(case):
    rows, cols, col0, kind, ld = case
    x = rk.case_values(rows, col0 + cols, kind)[:, col0:]
    _quarter(case, x)


@pytest.mark.parametrize("kind", rk.KINDS)
def test_emulation_within_a_quarter_on_the_special_columns(kind):
    x = rk.special_values(kind)
    _quarter(("special", kind), x)
    emu = rk.emulate_moments([x])
    assert torch.isfinite(emu["m2"]).all() and torch.isfinite(emu["mean"]).all()
    # the constant column: M2 and std exactly 0, and w the reference's own t_std / 1e-8
    assert float(emu["m2"][1]) == 0.0 and float(emu["std"][1]) == 0.0
    assert float(emu["mean"][1]) == float(x[0, 1])
    w, _ = rk.emulate_fit(emu, target_std=EMBED_INIT_RANGE, target_mean=0.0)
    w64, _ = rk.scale_to_ref(x, target_stds=torch.full((4,), EMBED_INIT_RANGE, dtype=F64), target_means=torch.zeros(4, dtype=F64))
    assert float(w[1]) == float(w64[0, 1].to(torch.float32)) == float(torch.tensor(EMBED_INIT_RANGE / 1e-8, dtype=torch.float32))


def test_emulation_of_three_unequal_calls_within_a_quarter():
    x = rk.case_values(2 * rk.CHUNK + 1, 9, "bf16", seed=3)
    cuts = [x[:70], x[70:70], x[70:]]
    _quarter("three calls", x, calls=[c for c in cuts])


def test_naive_formula_exceeds_the_std_bound():
    """The sensitivity case: mean 3, std 0.01, 4096 rows in fp32.  E[x^2] - mean^2 in fp32 must be OVER the std bound, the kernel's
    recurrence far under it."""
    x = rk.special_values("f32")[:, :1]
    assert x.shape[0] == 4096
    ref = rk.moments_ref(x)
    assert abs(float(ref["mean"]) - 3.0) < 1e-3 and abs(float(ref["std"]) - 0.01) < 5e-4
    bnd = rk.moments_bound(x, ref)
    naive = rk.emulate_naive(x)
    r_naive = _ratio(naive["std"], ref["std"], bnd["std"])
    r_kernel = _ratio(rk.emulate_moments([x])["std"], ref["std"], bnd["std"])
    print(f"std: naive err / bound {r_naive:.2f}, recurrence err / bound {r_kernel:.4f}, bound {float(bnd['std']):.3e}")
    assert r_naive > 1.0, r_naive
    assert r_kernel <= 0.25, r_kernel


def test_scale_to_ref_is_the_reference_formula():
    g = torch.Generator().manual_seed(5)
    x, t = torch.randn(50, 6, generator=g, dtype=F64) * 3 + 1, torch.randn(40, 6, generator=g, dtype=F64) * 0.02 - 0.1
    w, b = rk.scale_to_ref(x, t)
    y = x * w + b
    assert w.shape == b.shape == (1, 6)
    assert torch.allclose(y.mean(0), t.mean(0), atol=1e-12) and torch.allclose(y.std(0, unbiased=False), t.std(0, unbiased=False), rtol=1e-6)


def test_pairwise_cover():
    cases = rk.pairwise_cases()
    assert (4097, 520, 0, "bf16", 520) in cases
    cols = list(zip(*cases[:-1]))
    for a in range(4):
        for b in range(a + 1, 4):
            assert len(set(zip(cols[a], cols[b]))) == len(set(cols[a])) * len(set(cols[b])), (a, b)
    for kind in rk.KINDS:          # each element type with a 16-byte aligned and an unaligned first column
        es = 4 if kind == "f32" else 2
        al = {(c[2] * es) % 16 == 0 and (c[4] * es) % 16 == 0 for c in cases if c[3] == kind}
        assert al == {True, False}, kind


# ---- init_hypernet_state: host logic ----------------------------------------------------------------------------------------------
def _tiny(**over):
    cfg, *_ = synth.workload("tiny")
    cfg.update(over)
    return ZettHypernet(ZettHypernetConfig(**cfg))


def test_split_pretrained_state_drops_the_reference_list():
    state = {n: torch.zeros(1) for n in (
        "fallback_embeddings.weight", "input_projection.0.weight", "input_projection.0.bias", "output_projection.0.dense1.weight",
        "output_projection.1.bias", "output_projection_out.1.bias", "bias_projection.weight", "scaler.w", "scaler.b", "in_scaler.w",
        "out_scaler.w", "out_scaler.b", "model.encoder.layer.0.attention.self.query.weight", "model.embeddings.LayerNorm.bias")}
    kept, dropped = training.split_pretrained_state(state, True)
    assert dropped == ["fallback_embeddings.weight", "input_projection.0.weight", "input_projection.0.bias", "output_projection.0.dense1.weight",
                       "output_projection.1.bias", "bias_projection.weight", "scaler.w", "scaler.b", "in_scaler.w"]
    # the reference's list has no out_scaler, and matches whole components: output_projection_out is not output_projection
    assert list(kept) == ["output_projection_out.1.bias", "out_scaler.w", "out_scaler.b", "model.encoder.layer.0.attention.self.query.weight",
                          "model.embeddings.LayerNorm.bias"]
    kept, dropped = training.split_pretrained_state(state, False)
    assert dropped == [] and list(kept) == list(state)


def test_init_hypernet_state_overlays_on_a_model_without_rescalers():
    model = _tiny(hn_rescale_embeddings=False)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    assert not any("scaler" in n for n in before)
    src = torch.zeros(4, model.dims.n_in_embd)
    ids = torch.zeros(2, 7, dtype=torch.int32)
    assert training.init_hypernet_state(model, src, ids) == []
    new = {"input_projection.0.bias": torch.full_like(before["input_projection.0.bias"], 0.5),
           "model.embeddings.LayerNorm.bias": torch.full_like(before["model.embeddings.LayerNorm.bias"], -2.0)}
    dropped = training.init_hypernet_state(model, src, ids, pretrained_state=new, reinit_projectors=True)
    assert dropped == ["input_projection.0.bias"]
    after = dict(model.named_parameters())
    assert torch.equal(after["model.embeddings.LayerNorm.bias"], new["model.embeddings.LayerNorm.bias"])
    assert torch.equal(after["input_projection.0.bias"], before["input_projection.0.bias"])
    assert training.init_hypernet_state(model, src, ids, pretrained_state=new) == []
    assert torch.equal(dict(model.named_parameters())["input_projection.0.bias"], new["input_projection.0.bias"])
    with pytest.raises(KeyError, match="no_such"):
        training.init_hypernet_state(model, src, ids, pretrained_state={"no_such.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="shape"):
        training.init_hypernet_state(model, src, ids, pretrained_state={"input_projection.0.bias": torch.zeros(3)})


def test_init_rescaler_without_rescale_changes_no_parameter():
    model = _tiny(hn_rescale_embeddings=False)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    versions = {n: p._version for n, p in model.named_parameters()}
    assert model.init_rescaler(torch.zeros(2, 7, dtype=torch.int32), torch.zeros(4, model.dims.n_in_embd)) is None
    for n, p in model.named_parameters():
        assert torch.equal(p, before[n]) and p._version == versions[n], n


def test_fresh_rescalers_and_the_shared_constant():
    import inspect
    assert EMBED_INIT_RANGE == 0.02
    assert "std=EMBED_INIT_RANGE" in inspect.getsource(ZettHypernet._reset_parameters)
    assert "target_std=EMBED_INIT_RANGE" in inspect.getsource(ZettHypernet.init_rescaler)
    with pytest.raises(RuntimeError, match="MI355X only"):
        _tiny().init_rescaler(torch.zeros(2, 7, dtype=torch.int32), torch.zeros(4, 128))


def test_python_surface_refuses_before_any_launch():
    with pytest.raises(ValueError, match="device tensor"):
        training.column_moments(torch.zeros(4, 4))
    m = training.ColumnMoments(torch.zeros(5, 3, dtype=F64))
    assert m.cols == 5 and m.columns(1, 3).state.shape == (2, 3) and m.columns(1, 3).state.data_ptr() == m.state.data_ptr() + 24
    with pytest.raises(ValueError, match="outside"):
        m.columns(3, 6)
    with pytest.raises(ValueError, match="either target"):
        training.rescaler_fit(m)
    with pytest.raises(ValueError, match="either target"):
        training.rescaler_fit(m, m, target_std=1.0, target_mean=0.0)
    with pytest.raises(ValueError, match="either target"):
        training.rescaler_fit(m, target_std=1.0)
    with pytest.raises(ValueError, match="columns"):
        training.rescaler_fit(m, m.columns(0, 2))
    with pytest.raises(ValueError, match="ColumnMoments"):
        training.rescaler_fit(training.ColumnMoments(torch.zeros(5, 3)), target_std=1.0, target_mean=0.0)
    with pytest.raises(ValueError, match="MI355X only"):
        training.rescaler_fit(m, target_std=1.0, target_mean=0.0)


# ---- the C ABI surface ------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "zett_hip.h")).read(), flags=re.S)


def test_chunk_constant():
    assert training.COL_MOMENTS_CHUNK == _lib.COL_MOMENTS_CHUNK == rk.CHUNK == 256
    assert re.search(r"#define ZETT_COL_MOMENTS_CHUNK 256\b", open(os.path.join(REPO, "include", "zett_hip.h")).read())
    assert _lib.ABI_VERSION == 8 and _lib.load().zett_abi_version() == 8


@pytest.mark.parametrize("name", NEW)
def test_header_binding_and_library_agree(name):
    assert name in _lib.ABI_SYMBOLS
    params = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), re.S).group(1)
    fn = getattr(_lib.load(), name)
    want = ["ptr" if "*" in p else {"int64_t": C.c_int64, "int32_t": C.c_int32, "double": C.c_double}[p.split()[0]] for p in (q.strip() for q in params.split(","))]
    assert len(fn.argtypes) == len(want), (name, len(fn.argtypes), len(want))
    for i, (have, w) in enumerate(zip(fn.argtypes, want)):
        if w == "ptr":
            assert have is C.c_void_p or issubclass(have, C._Pointer), (name, i, have)
        elif w is C.c_double:
            assert have is C.c_double, (name, i, have)
        else:
            assert C.sizeof(have) == C.sizeof(w) and have(-1).value == -1, (name, i, have)


def test_entry_points_refuse_bad_arguments_before_touching_the_device():
    """No GPU needed: nothing is launched.  The return code says what kind of error, zett_last_error why."""
    lib = _lib.load()
    P = C.c_void_p
    buf = (C.c_double * 4096)()
    a, null = C.cast(buf, P), P(0)
    odd = P(C.addressof(buf) + 2)

    def refused(rc, *words):
        assert rc == _lib.E_INVALID, rc
        msg = lib.zett_last_error().decode()
        assert all(w in msg for w in words), msg

    need = C.c_int64(0)
    assert lib.zett_op_col_moments_workspace_bytes(2 * 256 + 1, 7, C.byref(need)) == 0 and need.value == 3 * 2 * 7 * 8
    assert lib.zett_op_col_moments_workspace_bytes(0, 1, C.byref(need)) == 0 and need.value == 16
    refused(lib.zett_op_col_moments_workspace_bytes(-1, 7, C.byref(need)), "rows = -1")
    refused(lib.zett_op_col_moments_workspace_bytes(5, 0, C.byref(need)), "cols = 0")
    refused(lib.zett_op_col_moments_workspace_bytes(5, 7, None), "shape")
    F = _lib.DTYPE_F32
    refused(lib.zett_op_col_moments(null, F, 16, 8, 0, 8, a, 0, a, 4096, null), "null")
    refused(lib.zett_op_col_moments(a, F, 16, 8, 0, 8, null, 0, a, 4096, null), "null")
    refused(lib.zett_op_col_moments(a, F, 16, 8, 0, 8, a, 0, null, 4096, null), "null")
    refused(lib.zett_op_col_moments(a, 7, 16, 8, 0, 8, a, 0, a, 4096, null), "dtype 7")
    refused(lib.zett_op_col_moments(a, F, 16, 8, 0, 0, a, 0, a, 4096, null), "cols = 0")
    refused(lib.zett_op_col_moments(a, F, 16, -1, 0, 8, a, 0, a, 4096, null), "rows = -1")
    refused(lib.zett_op_col_moments(a, F, 16, 8, -1, 8, a, 0, a, 4096, null), "col0 = -1")
    refused(lib.zett_op_col_moments(a, _lib.DTYPE_BF16, 16, 8, 9, 8, a, 0, a, 4096, null), "[9, 17)", "leading dimension 16")
    refused(lib.zett_op_col_moments(a, F, 16, 600, 0, 8, a, 0, a, 3 * 2 * 8 * 8 - 8, null), "workspace holds")
    refused(lib.zett_op_col_moments(odd, F, 16, 8, 0, 8, a, 0, a, 4096, null), "misaligned")
    refused(lib.zett_op_col_moments(a, F, 16, 8, 0, 8, odd, 0, a, 4096, null), "misaligned")
    refused(lib.zett_op_rescaler_fit(null, 8, null, 0.02, 0.0, a, a, null), "null")
    refused(lib.zett_op_rescaler_fit(a, 8, null, 0.02, 0.0, null, a, null), "null")
    refused(lib.zett_op_rescaler_fit(a, 8, null, 0.02, 0.0, a, null, null), "null")
    refused(lib.zett_op_rescaler_fit(a, 0, null, 0.02, 0.0, a, a, null), "cols = 0")
    refused(lib.zett_op_rescaler_fit(odd, 8, null, 0.02, 0.0, a, a, null), "misaligned")
    refused(lib.zett_op_rescaler_fit(a, 8, odd, 0.02, 0.0, a, a, null), "misaligned")


def test_the_unit_stays_out_of_the_forward_hash():
    from zett_amd import build
    assert "train_init.hip" in build.SOURCES and "train_init.hip" in build.TRAINING_ONLY
