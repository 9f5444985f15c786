"""CPU checks of tests/optimizer_ref.py on the exact inputs tests/test_gpu_optimizer.py uses: the f32 restatement of an
Adam step stays inside the bounds, an f32 accumulation of the finish test's partials does not, the layout references say
what test_pack_weights expects -- and the argument checks of the tail's entry points, which return before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import disyolo_oracle as O
import optimizer_ref as OR
from disyolo_amd import lib as L


# ------------------------------------------------------------------------------------------------ the Adam bounds
def sweep_cases():
    """(n, seed, n_decay, t) of every sweep the GPU tests judge; slice offsets do not change the values"""
    n = OR.CAP_N
    inside = 4 * (2048 * 256 + 1000) + 2           # inside a 16-byte vector of the second grid-stride iteration
    cases = [(n, 0, nd, t) for nd in (n, 0, inside, inside + 3) for t in (1, 7)]
    cases += [(c, 10 + i, c, 2) for i, c in enumerate(OR.SLICES)]
    return cases


@pytest.mark.parametrize("n,seed,n_decay,t", sweep_cases())
def test_f32_restatement_of_a_step_is_inside_the_bounds(n, seed, n_decay, t):
    w, g, m, v = OR.adam_inputs(n, seed)
    r = OR.adam_ref(w, g, m, v, t, n_decay)
    wr, mr, vr = OR.adam_f32(w, g, m, v, t, n_decay)
    OR.assert_step_within_bounds(wr, mr, vr, r, "f32 restatement")
    assert_extra_terms_vanish_without_cancellation(r, n)


def test_f32_restatement_of_the_first_step_from_zero_moments_is_inside_the_bounds():
    """adam_step_dev's first step, and what assert_swept_once holds the network's first step to"""
    w, g, m, v = OR.step_dev_inputs()
    r = OR.adam_ref(w, g, m, v, 1, OR.STEP_DEV_DECAY)
    OR.assert_step_within_bounds(*OR.adam_f32(w, g, m, v, 1, OR.STEP_DEV_DECAY), r, "f32 restatement")
    assert_extra_terms_vanish_without_cancellation(r, len(w))


def assert_extra_terms_vanish_without_cancellation(r, n):
    """the extra terms are what cancellation in g' lets through and nothing else: where g*gs and l2*w have one sign (and
    beyond n_decay) the bounds are the plain 2^-21 ones"""
    xm, xv = OR.cancellation(r)
    same = r["cancel_g"] <= 0
    assert same.sum() > n // 8 or n < 16
    assert (xm[same] == 0).all() and (xv[same] == 0).all()
    # and where they do cancel the terms stay what the count gives: u and 2u of the operands, never more
    gp, ops = np.abs(r["gp"]), np.abs(r["gp"]) + np.maximum(r["cancel_g"], 0)
    assert (xm <= (1 - OR.B1) * OR.U * ops).all() and (xv <= (1 - OR.B2) * (2 * OR.U * gp * ops + 9 * OR.U ** 2 * ops ** 2)).all()


def test_bounds_reject_a_wrong_moment_and_a_wrong_decay_flag():
    """what the bounds are for: a second sweep, a missed l2 term and a wrong bias correction are far outside them"""
    n = 4099
    w, g, m, v = OR.adam_inputs(n, 3)
    r = OR.adam_ref(w, g, m, v, 7, 1030)
    ok = OR.adam_f32(w, g, m, v, 7, 1030)
    OR.assert_step_within_bounds(*ok, r)
    bm, bv, bw = OR.adam_bounds(r)
    flag = OR.adam_f32(w, g, m, v, 7, 1031)                       # one element more gets l2*w
    assert OR.worst(flag[1], r["m"], bm)[0] > 10 and OR.worst(flag[1], r["m"], bm)[1] == 1030
    t8 = OR.adam_f32(w, g, m, v, 8, 1030)                         # the next step's bias correction
    assert OR.worst(t8[0], r["w"], bw)[0] > 10
    twice = OR.adam_f32(ok[0], g, ok[1], ok[2], 7, 1030)
    assert OR.worst(twice[1], r["m"], bm)[0] > 1e3 and OR.worst(twice[2], r["v"], bv)[0] > 1e3


def test_reference_step_is_the_oracles_tf_form():
    w, g, m, v = OR.adam_inputs(7, 1)
    r = OR.adam_ref(w, g, m, v, 3, 4, grad_scale=0.5)
    gp = g.astype(np.float64) * 0.5
    gp[:4] += OR.L2 * w[:4].astype(np.float64)
    tw, tm, tv = O.adam_tf_step(torch.from_numpy(w.astype(np.float64)), torch.from_numpy(gp), torch.from_numpy(m.astype(np.float64)),
                                torch.from_numpy(v.astype(np.float64)), 3, lr=OR.LR, b1=OR.B1, b2=OR.B2, eps=OR.EPS)
    assert np.array_equal(r["w"], tw.numpy()) and np.array_equal(r["m"], tm.numpy()) and np.array_equal(r["v"], tv.numpy())
    assert OR.l2_term(w, 4) == 0.5 * OR.L2 * float((w[:4].astype(np.float64) ** 2).sum())


# ------------------------------------------------------------------------------------------------ the finish
@pytest.mark.parametrize("nparts", OR.FINISH_NPARTS)
def test_finish_partials_defeat_an_f32_accumulation(nparts):
    p = OR.finish_parts(nparts)
    assert p.dtype == np.float32 and len(p) == nparts
    want = OR.finish_ref(p)
    # a double accumulation rounded once is inside the bound, in any order
    for order in (p, p[::-1], np.sort(p)):
        got = float(np.float32(np.asarray(order, np.float64).sum() * (0.5 * OR.L2)))
        assert abs(got - want) <= OR.FINISH_REL * want
    if nparts >= 255:
        assert p.min() == np.float32(1e-8) and p.max() == np.float32(1e4)
        got = float(np.float32(np.float64(OR.f32_running_sum(p)) * (0.5 * OR.L2)))
        assert abs(got - want) > OR.FINISH_REL * want, "an f32 running sum would pass the finish test at nparts = %d" % nparts


def test_thread_sum_bound_counts_the_elements_of_one_thread():
    assert OR.sweep_blocks(OR.CAP_N) == 2048 and OR.sweep_blocks(5000) == 5 and OR.sweep_blocks(3) == 1
    assert OR.thread_sum_rel(OR.CAP_N, 2048) == 19 * 2.0 ** -24       # two float4 and one trailing scalar
    assert OR.l2_blocks(OR.L2_NS[2]) == 1024 and OR.l2_blocks(2047) == 1 and OR.l2_blocks(2049) == 2
    assert OR.thread_sum_rel(OR.L2_NS[2], 1024) == 27 * 2.0 ** -24
    # the existing fused test's 2e-6 at its 4099 elements: 5 blocks, 4 elements a thread, plus the finish
    assert OR.thread_sum_rel(4099, OR.sweep_blocks(4099)) + OR.FINISH_REL < 2e-6


# ------------------------------------------------------------------------------------------------ layouts
def test_layout_references_agree_with_test_pack_weights():
    g = torch.Generator().manual_seed(5)
    for k, cin, cout, pad in ((3, 64, 128, 128), (1, 96, 24, 32), (3, 32, 9, 32)):
        w = torch.randn(k, k, cin, cout, generator=g)
        # test_gpu_conv.test_pack_weights' expectations, verbatim
        assert torch.equal(OR.fwd_layout(w), w.permute(3, 0, 1, 2).reshape(cout, k * k * cin))
        ref = torch.zeros(cin, k, k, pad)
        ref[..., :cout] = w.flip(0, 1).permute(2, 0, 1, 3)
        assert torch.equal(OR.dgrad_layout(w, pad), ref.reshape(cin, -1))
        # element by element, as the header words it
        d = OR.dgrad_layout(w, pad).view(cin, k * k, pad)
        wt = w.reshape(k * k, cin, cout)
        for ci, tp, co in ((0, 0, 0), (cin - 1, k * k - 1, cout - 1), (cin // 2, (k * k) // 2, cout // 3)):
            assert d[ci, tp, co] == wt[k * k - 1 - tp, ci, co]
        assert (d[..., cout:] == 0).all()


def test_pack_inputs_and_block_count():
    jobs = OR.PACK_JOBS
    # forward 64 x 64 tiles + 4096-element data-gradient chunks, job by job
    assert [OR.pack_blocks([j]) for j in jobs] == [16 * 2, 2 * 1 + 1, 1 + 1, 9 * 2 + 18, 5 * 1 + 3, 1 + 1, 2 * 1]
    assert OR.pack_blocks(jobs) == 32 + 3 + 2 + 36 + 8 + 2 + 2
    assert 64 * 1 * 64 == 4096                                        # job 2: exactly one full data-gradient chunk
    seen = []
    for i, (k, cin, cout, pad, dg) in enumerate(jobs):
        w = OR.pack_weights_for(i)
        assert w.shape == (k, k, cin, cout) and w.dtype == torch.float32
        a = w.abs().flatten()
        bulk = a[(a >= i + 1.25) & (a < i + 1.75)]
        assert bulk.numel() >= a.numel() - 24 and bulk.numel() > 0.5 * a.numel()
        seen.append((float(bulk.min()), float(bulk.max())))
        flat = w.flatten()
        zeros = flat[flat == 0]
        assert torch.signbit(zeros).any() and (~torch.signbit(zeros)).any()          # -0 and +0
        # exact ties: the two bf16 neighbours are equally far, and nearest-even goes each way for each sign
        r = flat.to(torch.bfloat16).float()
        up, down = 2.0 * flat - r, r                                                  # the other neighbour mirrors r
        tie = (flat != r) & (up.to(torch.bfloat16).float() == up) & ((up - flat) == (flat - down))
        assert ((r > flat) & tie & (flat > 0)).any() and ((r < flat) & tie & (flat > 0)).any()
        assert ((r > flat) & tie & (flat < 0)).any() and ((r < flat) & tie & (flat < 0)).any()
    for (lo, hi), (lo2, _) in zip(seen, seen[1:]):
        assert hi < lo2                                                               # disjoint per job


# ------------------------------------------------------------------------------------------------ argument checks
def test_tail_entry_points_reject_bad_arguments_before_any_launch():
    """host buffers stand in for device memory: a launch would fault on them, the checks return first"""
    lib = L.load()
    raw = ctypes.create_string_buffer(1 << 12)
    base = (ctypes.addressof(raw) + 63) & ~63
    p = lambda off=0: ctypes.c_void_p(base + off)
    err = lambda: lib.disyolo_last_error()

    def sweep(w=p(0), g=p(256), m=p(512), v=p(768), n=8, n_decay=8, parts=None):
        return lib.disyolo_adam_sweep(w, g, m, v, n, n_decay, p(1024), 0.9, 0.999, 1e-8, 5e-4, p(1088), 1.0, parts, None)

    assert sweep(m=p(512 + 4)) == -1 and b"adam_sweep" in err() and b"same offset" in err()
    assert sweep(g=p(256 + 8)) == -1 and b"adam_sweep" in err()
    assert sweep(w=p(4), g=p(260), m=p(516), v=p(772 + 4)) == -1 and b"adam_sweep" in err()
    assert sweep(n_decay=9) == -1 and b"adam_sweep" in err()
    assert lib.disyolo_adam_finish(p(1088), None, 0, 5e-4, p(1152), None) == -1 and b"adam_finish" in err()
    assert lib.disyolo_adam_finish(p(1088), p(0), 0, 5e-4, p(1152), None) == -1 and b"adam_finish" in err()

    jobs = (L.PackJob * 2)(L.PackJob(base, base + 256, None, 1, 8, 8, 8), L.PackJob(base, None, base + 512, 1, 8, 8, 8))
    host = ctypes.create_string_buffer(lib.disyolo_pack_table_bytes(2))
    blocks = ctypes.c_int(-7)
    assert lib.disyolo_pack_table_build(jobs, 2, host, ctypes.byref(blocks)) == -1
    assert b"pack_table_build" in err() and b"job 1" in err()
    assert lib.disyolo_pack_table_build(jobs, 1, host, ctypes.byref(blocks)) == 0 and blocks.value == 1
    assert lib.disyolo_pack_all(p(0), 1, 0, None) == -1 and b"pack_all" in err()
