"""The GEMM checker (tests/gemm_check.py) fails a subtly wrong kernel, and passes a right one (no GPU).

A right kernel is the fp32 emulation of gemm_check.emulate: K accumulated in chunks of 4, fp32 epilogue.  Every fault a tile
kernel could plausibly have is then injected into that result, one at a time, and must be flagged AT ITS ELEMENT: the mask of
elements over their bound and the lists of rows / columns over the slice limit name exactly the damaged part, nothing else.
"""
import pytest
import torch

from tests import gemm_check as gc

M, N, LD_RES = 37, 24, 32          # more than one 8-column group, odd row count, a residual with padding columns
KS = (64, 512, 2112)
KINDS = ("f32", "bf16", "f16")

_CASES = {}


def _case(kind, k):
    """operands, a residual stored with leading dimension LD_RES (finite padding), and the emulated accumulator — made once"""
    if (kind, k) not in _CASES:
        a, w, bias, _ = gc.operands(kind, M, N, k, seed=1000 + k)
        g = torch.Generator().manual_seed(k)
        res_store = torch.randn(M, LD_RES, generator=g)
        _CASES[kind, k] = (a, w, bias, res_store, gc.emulate_acc(a, w))
    return _CASES[kind, k]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", KINDS)
def test_clean_emulation_passes_every_epilogue(kind, k):
    a, w, bias, res_store, acc = _case(kind, k)
    res = res_store[:, :N]
    for act in (0, 1, 2):
        for b in (None, bias):
            for r in (None, res):
                ref = gc.reference(a, w, b, act, r)
                ratio, rel = gc.check(gc.emulate_epilogue(acc, b, act, r), ref, k, act, f"emulation {kind} k={k} act={act}")
                assert ratio <= 0.04, (kind, k, act, ratio)          # the derived bound is 25x what rounding really does
                assert rel <= gc.SLICE_REL


def test_one_element_slices_are_held_per_element():
    """m = 1: a column is one element, and its relative error is unbounded under cancellation for ANY fp32 arithmetic (the clean
    emulation has elements beyond 2e-6 here): those slices are held by the per-element bound, the row by both."""
    a, w, bias, res = gc.operands("f32", 1, 520, 64, seed=2)
    ref = gc.reference(a, w, bias, 0, res)
    got = gc.emulate(a, w, bias, 0, res)
    assert float(((got.double() - ref["y"]).abs() / ref["y"].abs()).max()) > gc.SLICE_REL       # why the rule exists
    gc.check(got, ref, 64, 0, "m = 1")
    got[0, 300] += 4 * float(gc.bound(ref, 64, 0)[0, 300])
    with pytest.raises(gc.GemmMismatch) as e:
        gc.check(got, ref, 64, 0, "m = 1, one element off")
    assert (e.value.row, e.value.col) == (0, 300) and int(e.value.bad.sum()) == 1


def _flagged(got, ref, k, act, what):
    with pytest.raises(gc.GemmMismatch) as e:
        gc.check(got, ref, k, act, what)
    return e.value


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("kind", KINDS)
def test_injected_faults_are_flagged_at_their_element(kind, k):
    a, w, bias, res_store, acc = _case(kind, k)
    res = res_store[:, :N].contiguous()
    a64, w64 = a.double(), w.double()
    ref = gc.reference(a, w, bias, 0, res)
    good = gc.emulate_epilogue(acc, bias, 0, res)
    gc.check(good, ref, k, 0, "clean")

    # one 8-wide K chunk missing from a single element (the chunk that weighs most there: a dropped chunk of products that
    # cancel is not a wrong result)
    i, j = 19, 13
    parts = (a64[i] * w64[j]).view(-1, 8).sum(1)
    got = good.clone()
    got[i, j] = float(good[i, j].double() - parts[int(parts.abs().argmax())])
    e = _flagged(got, ref, k, 0, "K chunk missing")
    assert (e.row, e.col) == (i, j) and int(e.bad.sum()) == 1 and e.rows in ([], [i]) and e.cols in ([], [j])

    # the last K step (128 bytes of K) missing from the last row
    step = gc.K_STEP[kind]
    got = good.clone()
    got[M - 1] = (good[M - 1].double() - a64[M - 1, k - step:] @ w64[:, k - step:].T).float()
    e = _flagged(got, ref, k, 0, "last K step missing")
    assert e.row == M - 1 and bool(e.bad[M - 1].any()) and not bool(e.bad[:M - 1].any()) and e.rows == [M - 1]

    # two adjacent output columns swapped inside one 8-column group
    got = good.clone()
    got[:, [10, 11]] = good[:, [11, 10]]
    e = _flagged(got, ref, k, 0, "columns swapped")
    assert e.col in (10, 11) and e.cols == [10, 11] and not bool(e.bad[:, :10].any()) and not bool(e.bad[:, 12:].any())

    # bias missing on the last column
    got = good.clone()
    got[:, N - 1] = good[:, N - 1] - bias[N - 1]
    e = _flagged(got, ref, k, 0, "bias missing")
    assert e.cols == [N - 1] and not bool(e.bad[:, :N - 1].any())

    # bias shifted by one
    shifted = torch.cat([bias[1:], bias[:1]])
    e = _flagged(gc.emulate_epilogue(acc, shifted, 0, res), ref, k, 0, "bias shifted")
    assert e.cols == list(range(N)) and e.rows == list(range(M))

    # residual read with leading dimension n instead of ld_res: row 0 is right, every other row reads across the padding
    wrong = res_store.flatten()[:M * N].view(M, N)
    e = _flagged(gc.emulate_epilogue(acc, bias, 0, wrong), ref, k, 0, "residual leading dimension")
    assert e.rows == list(range(1, M)) and not bool(e.bad[0].any()) and e.row >= 1

    # row m - 1 equal to row m - 2
    got = good.clone()
    got[M - 1] = good[M - 2]
    e = _flagged(got, ref, k, 0, "row repeated")
    assert e.rows == [M - 1] and e.row == M - 1 and not bool(e.bad[:M - 1].any())

    # tanh-GELU where erf was asked: at most 5e-4 per element (under the element bound of a long K) — the slices see it
    ref2 = gc.reference(a, w, bias, 2, res)
    gc.check(gc.emulate_epilogue(acc, bias, 2, res), ref2, k, 2, "clean erf")
    e = _flagged(gc.emulate_epilogue(acc, bias, 1, res), ref2, k, 2, "wrong GELU")
    assert e.rows == list(range(M)) and e.cols == list(range(N))


def test_canary_names_a_write_past_the_output():
    frame = gc.Framed(M, N, N + 4, torch.float32, "canary")
    buf = frame.buf.clone()
    with pytest.raises(AssertionError, match="not finite"):          # nothing written yet: the canary is a NaN
        gc.check_canary(frame, buf, "unwritten")
    frame.view(buf).copy_(torch.randn(M, N))
    gc.check_canary(frame, buf, "clean")
    one = buf.clone()
    one[frame.offset + 5 * frame.ld + N] = 1.0          # one column past n in row 5: element (5, N) of the [M, ld] layout
    with pytest.raises(gc.CanaryBroken) as e:
        gc.check_canary(frame, one, "one column past n")
    assert e.value.where == [(5, N)]
    two = buf.clone()
    two[frame.offset + M * frame.ld + 3] = 0.0
    with pytest.raises(gc.CanaryBroken) as e:
        gc.check_canary(frame, two, "one row past m")
    assert e.value.where == [(M, 3)]
    three = buf.clone()
    three[frame.offset - 1] = 2.0                                    # the last element in front of the view
    with pytest.raises(gc.CanaryBroken) as e:
        gc.check_canary(frame, three, "in front")
    assert e.value.where == [(-1, frame.ld - 1)]
    # a value equal to the canary's float value but other bits does not pass for it: the comparison is on bits
    four = buf.clone()
    four.view(torch.int32)[frame.offset + M * frame.ld] = 0x7FC00000
    with pytest.raises(gc.CanaryBroken):
        gc.check_canary(frame, four, "another NaN")
    vec = gc.Framed(None, N, N, torch.float32, "canary")
    v = vec.buf.clone()
    vec.view(v).fill_(1.0)
    v[vec.offset + N] = 1.0
    with pytest.raises(gc.CanaryBroken) as e:
        gc.check_canary(vec, v, "vector")
    assert e.value.where == [(0, N)]
