"""Every single-call switch on at once, on a real MI355X: xsmm_hip_set_dma256_edge, _edge_tiles, _edge_k, _edge_k_bf16, _edge_k8_bf16,
_dma256_images, _tail_split and _f32_halves all set to one context - "rule" (every switch at its rule value, the edge tiles at 2) or
"eligible" (mode 2 where it exists, tail_split 2) - and one whole-layer call per row of tests/call_switches_worker.py ROWS: the smallest shape of
each form plan_gemm_call refines, the shapes several switches compete for (256 x 264 x 96: the 256x256 edge tile, bf16 ragged k and the edge
tiles; 264 x 264 x 72: refused by the 256x256 edge tile for its k, lands on "edge tiles, ragged k, half step"), and calls every switch must
leave alone (divisible shapes, a forced variant, the forced generic kernel, a VNNI C, a C pointer off 16 bytes, a forced split count).
What each row must report is hard-coded there; tests/test_gemm_call_switches.py pins that it is the planner's P(all) at 64, 256 and 304
compute units. Per row and context:
  1 exact inputs (tests/exact_data.py), bias + relu at beta 0 and plain at beta 1, strided operands, moved base pointers, NaN in every gap
    and a bit pattern around C: the oracle equals the fp64 result rounded once (the precondition), the kernel equals the oracle bit for bit,
    the surroundings are intact, the outputs finite; xsmm_hip_last_refined_kernel is the expected text; exactly the winner's counter moved by
    one and every other single-call counter and every chain counter stands still
  2 random operands: the bits under the full set are the bits under the winner's read set alone (no winner: with every switch off) - the
    same kernel, the same order of additions, no tolerance
  3 a child process with the eight TPP_HIP_* variables and TPP_HIP_STRICT=1 gives three of the rows the same texts and digests (rows of more
    than 64 x 64 outputs: strict mode runs smaller single invokes as a group of one, which no single-call switch reaches)
The planner accepts nothing its launchers refuse (tests/test_gemm_call_switches.py, check d), so there is no fallback row.
The last test is the inventory: every text and every counter a row expects was reached. A fixture restores all eight modes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import call_switches_worker as csw
import exact_data as ed

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REACHED = set()   # (context, label, winner, text) of every row that passed
SEED = 20261


@pytest.fixture(scope="module")
def rt():
    r = csw.runtime()
    assert r.device_count() >= 1, "no HIP device visible: the gpu tests need an MI355X"
    return r


@pytest.fixture(params=sorted(csw.CONTEXTS))
def context(rt, request):
    """all eight modes set to one context, and all of them put back afterwards"""
    prev = csw.set_modes(rt, csw.CONTEXTS[request.param])
    assert all(v >= 0 for v in prev.values()), prev
    try:
        yield request.param
    finally:
        csw.set_modes(rt, prev)


def dtype_of(r):
    return ed.F32 if r["dt"] == csw.F32 else ed.BF16


@pytest.mark.parametrize("r", csw.ROWS, ids=[r["label"].split(":", 1)[1] for r in csw.ROWS])
def test_every_switch_on_at_once(rt, context, r):
    winner, text = r["expect"][context]
    want_moved = {winner: 1} if winner else {}
    what = "%s under %s" % (r["label"], context)
    # 1 exact inputs against the oracle
    if not r["vc"]:
        for beta0 in (True, False):
            case = csw.make_case(r, SEED + beta0, exact=True, beta0=beta0)
            ref = case.oracle()
            assert np.array_equal(ed.bits(ref[case.win]), ed.bits(case.fp64())), what + ": the oracle is not the fp64 result rounded once"
            got, refined, mv = csw.run_case(rt, r, case)
            assert refined == text, (what, refined)
            assert mv == want_moved, (what, mv)
            ed.check_bits(got[case.win], ref[case.win], dtype_of(r), "%s beta0=%d" % (what, beta0))
            assert case.outside_untouched(got), what + ": wrote outside the output window"
            assert np.isfinite(ed.as_f32(got[case.win])).all(), what
    # 2 random operands: the full set against the winner's read set alone
    case = csw.make_case(r, SEED + 7)
    full, refined, mv = csw.run_case(rt, r, case)
    assert refined == text and mv == want_moved, (what, refined, mv)
    alone = dict(csw.OFF, **{s: csw.CONTEXTS[context][s] for s in (csw.READS[winner] if winner else [])})
    prev = csw.set_modes(rt, alone)
    try:
        only, refined_only, mv_only = csw.run_case(rt, r, case)
    finally:
        csw.set_modes(rt, prev)
    assert refined_only == text and mv_only == want_moved, (what, alone, refined_only, mv_only)
    assert np.array_equal(ed.bits(full), ed.bits(only)), what + ": the bits under the full set differ from those under " + str(alone)
    if not r["vc"]:
        assert case.outside_untouched(full), what
    REACHED.add((context, r["label"], winner, text))


@pytest.mark.timeout(300)
def test_a_child_process_reads_all_eight_modes_and_strict_mode_from_the_environment(rt):
    ctx = "eligible"
    env = {k: v for k, v in os.environ.items() if not k.startswith("TPP_HIP_")}
    env.update({"TPP_HIP_" + s.upper(): str(v) for s, v in csw.CONTEXTS[ctx].items()}, TPP_HIP_STRICT="1")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "call_switches_worker.py"), str(SEED + 7)] + csw.ENV_ROWS, capture_output=True, text=True,
                       env=env, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    child = json.loads(p.stdout.strip().splitlines()[-1])
    assert child["modes"] == csw.CONTEXTS[ctx] and child["strict"] == 1, child
    prev = csw.set_modes(rt, csw.CONTEXTS[ctx])
    try:
        for label in csw.ENV_ROWS:
            r = csw.BY_LABEL[label]
            got, refined, mv = csw.run_case(rt, r, csw.make_case(r, SEED + 7))
            c = child["rows"][label]
            assert (c["kernel"], c["moved"]) == (refined, mv) == (r["expect"][ctx][1], {r["expect"][ctx][0]: 1}), (label, c, refined, mv)
            assert c["digest"] == csw.digest(got), label + ": other bits in the child process"
    finally:
        csw.set_modes(rt, prev)


def test_zz_every_refinement_a_row_expects_was_reached():
    want = {(ctx, r["label"], *r["expect"][ctx]) for r in csw.ROWS for ctx in csw.CONTEXTS}
    assert REACHED == want, sorted(want - REACHED)[:10]
    assert {w for _, _, w, _ in REACHED} == set(csw.SWITCHES) | {None}
    texts = {t for _, _, _, t in REACHED}
    for part in ("<256x256>, edge tiles", "_flatb<256x256>", "_vnni4<256x256>", "<32x64,k2>, edge tiles", ", ragged k", ", ragged k, half step",
                 ", edge tiles, ragged k", ", edge tiles, ragged k, half step", "brgemm_f32_lw<32x32,k4>, edge tiles", "brgemm_f32_lw<32x32,k4>, ragged k",
                 "brgemm_f32_lw<32x32,k4>, edge tiles, ragged k", ", tail split", ", split"):
        assert any(t.endswith(part) or part in t for t in texts), part
