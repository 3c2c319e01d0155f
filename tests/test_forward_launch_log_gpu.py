"""The forward's host orchestration against a recording of the commit before it was rewritten (tests/golden/forward_launch_log.json,
written by tests/golden/make_golden_forward_launch_log.py on that commit's library): per case of tests/forward_launch_cases.py the same
GEMM launches in the same order, the same stats(), the same workspace_bytes() and the same bytes in every output."""
import json
import os

import pytest

from tests import forward_launch_cases as cases

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_launch_log.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_covers_every_case():
    assert set(GOLDEN["cases"]) == set(cases.CASES)
    assert all(name in cases.CASES for name in GOLDEN["unreproducible"])
    for name, want in GOLDEN["cases"].items():
        assert want["gemm_log"] and (name in GOLDEN["unreproducible"] or want["outputs"][0] is not None), name


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_forward_matches_the_recorded_parent(name):
    want, got = GOLDEN["cases"][name], cases.run_case(name)
    assert got["gemm_log"] == want["gemm_log"]
    assert got["stats"] == want["stats"]
    assert got["workspace_bytes"] == want["workspace_bytes"]
    assert len(got["outputs"]) == len(want["outputs"])
    for g, w in zip(got["outputs"], want["outputs"]):
        if w is not None or name not in GOLDEN["unreproducible"]:          # (a digest the parent itself did not reproduce was dropped)
            assert g == w


def test_shared_table_reproduces_the_plain_forward():
    """(what the parent already guarantees, now on the recorded digests)"""
    assert GOLDEN["cases"]["shared_table"]["outputs"] == GOLDEN["cases"]["h512_default"]["outputs"]
    assert GOLDEN["cases"]["prepared"]["outputs"] == GOLDEN["cases"]["h512_default"]["outputs"]
    assert GOLDEN["cases"]["id_qkv_shared_table"]["outputs"] == GOLDEN["cases"]["id_qkv"]["outputs"]


def test_timing_the_launches_changes_neither_the_log_nor_the_outputs():
    for key in ("gemm_log", "stats", "workspace_bytes", "outputs"):
        assert GOLDEN["cases"]["h512_time_gemm"][key] == GOLDEN["cases"]["h512_default"][key], key
