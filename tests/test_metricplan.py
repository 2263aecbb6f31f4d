"""metricplan.MetricPlan on CPU tensors, without the library: where the regions lie and what the job tables hold after finalise()."""
import ctypes as C

import pytest
import torch

import _cabi
import gru_vae
from metricplan import RESULT, SCRATCH, MetricPlan, Ref

F = 8      # bytes of an arena element


def arena_span(plan, r):
    """[first, last) of a region in elements of the arena (results and scratch) or of the twf buffer"""
    at = r.off + (plan.n_out if r.seg == SCRATCH else 0)
    return at, at + r.rows * r.cols


@pytest.fixture(scope="module")
def built():
    plan = MetricPlan(torch.device("cpu"))
    x = torch.zeros(2, 9, 6, dtype=torch.float32)
    ext = torch.zeros(5, 4, dtype=torch.float64)
    r = {"s0": plan.vec(), "m0": plan.mat(7, 4), "v": plan.vec(5), "m1": plan.mat(9, 4), "s1": plan.vec(), "m2": plan.mat(3, 6)}
    plan.stat(1, _cabi.STAT_GATHER64, 7, 0, 4, x.data_ptr(), 6, idx=1234, dst=r["m0"], src_rows=9)
    plan.stat(2, _cabi.STAT_MCD64, 7, 1, 4, ext.data_ptr(), 4, r["m0"], 4, out=r["s1"], src_rows=5)
    r["al"] = plan.mat(9, 4)
    r["frames"] = plan.align(r["m0"], r["m1"], -1, aligned=r["al"], mean=r["s0"], c0=1)
    r["frames_ext"] = plan.align(r["m1"], plan.f64(ext), 0)
    r["ld"] = plan.latent_distance(r["m0"], r["m1"])
    plan.finalise()
    with pytest.MonkeyPatch.context() as mp:      # (begin() notes the library and the stream its steps will use: there is neither here)
        mp.setattr(gru_vae, "_lib", lambda: None)
        mp.setattr(gru_vae, "_stream", lambda: 0)
        plan.begin()
    return plan, r, x, ext


def test_regions_are_disjoint_and_inside_the_arena(built):
    plan, r, _, _ = built
    regions = [v for v in r.values() if isinstance(v, Ref)] + list(r["ld"])
    spans = {arena_span(plan, x) for x in regions}
    # what the plan took for itself, from the problems it built: aligned sequences, frame costs, mean costs
    el = lambda address: (address - plan.arena.data_ptr()) // F
    for q in plan.probs:
        spans |= {(el(q.frames), el(q.frames) + q.T2), (el(q.mean_out), el(q.mean_out) + 1)}
        if q.aligned is not None:
            spans.add((el(q.aligned), el(q.aligned) + q.T2 * q.ld_trg))
    spans = sorted(spans)
    assert len(spans) == 7 + 4 + 2 + 6 + 3          # declared, latent_distance's slots and aligned sequences, frames, unread means
    assert spans[0][0] == 0 and spans[-1][1] == plan.arena.numel()
    for (a0, a1), (b0, b1) in zip(spans, spans[1:]):
        assert a0 < a1 == b0, "regions overlap or leave a hole"
    # the results are [0, n_out): two scalars, the vector, the four slots of the latent distance; nothing else lies there
    assert plan.n_out == 2 + 5 + 4
    assert max(arena_span(plan, x)[1] for x in regions if x.seg == RESULT) == plan.n_out
    assert min(arena_span(plan, x)[0] for x in regions if x.seg == SCRATCH) == plan.n_out
    assert plan.results().data_ptr() == plan.arena.data_ptr() and plan.results().numel() == plan.n_out


def test_addresses_are_arena_offsets(built):
    plan, r, x, ext = built
    a0 = plan.arena.data_ptr()
    A = lambda ref: a0 + F * arena_span(plan, ref)[0]
    for ref in [v for v in r.values() if isinstance(v, Ref)] + list(r["ld"]):
        assert ref.addr == A(ref)
    j1, j2 = plan.table[0], plan.table[1]
    assert (j1.kind, j1.a, j1.dst, j1.idx, j1.lda, j1.src_rows, j1.out_off) == (_cabi.STAT_GATHER64, x.data_ptr(), A(r["m0"]), 1234, 6, 9, 0)
    assert (j2.kind, j2.a, j2.b, j2.c0, j2.c1, j2.out_off) == (_cabi.STAT_MCD64, ext.data_ptr(), A(r["m0"]), 1, 4, r["s1"].off)
    assert len(plan.table) == 2 + 2 and [j.kind for j in plan.table[2:]] == [_cabi.STAT_LATDIST] * 2
    # latent_distance: each aligned sequence against what it was aligned to, into the first two slots
    for j, trg, slot in zip(plan.table[2:], (r["m1"], r["m0"]), r["ld"][:2]):
        assert (j.b, j.rows, j.c1, j.lda, j.ldb, j.out_off) == (A(trg), trg.rows, 4, 4, 4, slot.off)
        assert plan.n_out <= (j.a - a0) // F < plan.arena.numel()
    assert plan.job_ptr(1) == plan.jdev.data_ptr() and plan.job_ptr(2) == plan.job_ptr(1) + 1 * C.sizeof(_cabi.StatJob)
    assert plan.jdev.numel() == 4 * C.sizeof(_cabi.StatJob) and bytes(plan.jdev.numpy()) == bytes(plan.table)


def test_alignments(built):
    plan, r, _, ext = built
    a0, w0 = plan.arena.data_ptr(), plan.twf.data_ptr()
    A = lambda ref: a0 + F * arena_span(plan, ref)[0]
    p = plan.probs
    assert len(p) == 2 + 4
    # c0 = 1: both operands one column on, D one less, the leading dimensions unchanged
    assert (p[0].org, p[0].trg, p[0].D, p[0].ld_org, p[0].ld_trg, p[0].T1, p[0].T2) == (A(r["m0"]) + F, A(r["m1"]) + F, 3, 4, 4, 7, 9)
    assert (p[0].aligned, p[0].mean_out, p[0].frames, p[0].mcd) == (A(r["al"]), A(r["s0"]), A(r["frames"]), -1)
    # an operand outside the arena is taken at its own address
    assert (p[1].org, p[1].trg, p[1].D, p[1].T2, p[1].aligned, p[1].mcd) == (A(r["m1"]), ext.data_ptr(), 4, 5, None, 0)
    # latent_distance: mel-cd with an aligned output, cosine into the slot, then the same pair the other way round
    assert [(q.org, q.trg, q.mcd, q.aligned is not None) for q in p[2:]] == [
        (A(r["m0"]), A(r["m1"]), -1, True), (A(r["m1"]), A(r["m0"]), 0, False), (A(r["m1"]), A(r["m0"]), -1, True), (A(r["m0"]), A(r["m1"]), 0, False)]
    assert [p[3].mean_out, p[5].mean_out] == [A(x) for x in r["ld"][2:]]
    # frames (T2 doubles in the scratch part) and twf rows (T2 int64 of the other buffer) of different problems do not overlap
    fr = sorted(((q.frames - a0) // F, (q.frames - a0) // F + q.T2) for q in p)
    tw = sorted(((q.twf - w0) // F, (q.twf - w0) // F + q.T2) for q in p)
    for spans, lo, hi in ((fr, plan.n_out, plan.arena.numel()), (tw, 0, plan.twf.numel())):
        assert spans[0][0] >= lo and spans[-1][1] <= hi
        assert all(a1 <= b0 for (_, a1), (b0, _) in zip(spans, spans[1:]))
    assert plan.twf.numel() == sum(q.T2 for q in p) and (plan.t1max, plan.t2max) == (9, 9)


def test_an_empty_plan_finalises():
    plan = MetricPlan(torch.device("cpu"))
    plan.finalise()
    plan.begin(pinned=True)
    assert plan.n_out == 0 and plan.arena.numel() == 1 and plan.twf.numel() == 1 and plan.results().numel() == 1
    assert len(plan.table) == 0 and len(plan.probs) == 0 and plan.jdev.numel() == 0 and plan.work_bytes == 0
    plan.stats(1)          # (nothing to launch: neither step looks for the library)
    plan.dtw()
    plan.stats(2)
