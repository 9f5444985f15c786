"""Any lock map on plan-only nets (CPU): the ``lock=`` overlay, the variables a holed map trains, the locked layers the
backward pass has to cross ("pass-through"), the fp8 refusal, and the data-parallel bucket plan over a holed arena.

The reference: ``lock`` is an argument of every conv_bn / conv call (yolo/yolo3_net_pos.py:71-146); the oracle takes any map."""
import os

import pytest
import torch

import disyolo_oracle as O
import mask_stride_ref as R
from disyolo_amd.net import YOLONet, build_topology
from lock_maps import MAPS, SCORE_LAYER, STRIDE_MAPS, inputs_of, lock_of, pass_through


def _net(name, **kw):
    m, lock = lock_of(name)
    return YOLONet(training=True, plan_only=True, mask_stride=m, lock=lock, **kw), m, lock


def test_lock_overlays_the_stage_default():
    net = YOLONet(training=True, plan_only=True, stage=1, lock={62: True, 63: True, 10: False})
    want = {i: i <= 52 for i in range(1, 83)}
    want.update({62: True, 63: True, 10: False})
    assert net.lock == want
    assert [l.lock for l in net.layers] == [want[i] for i in range(1, 83)]
    # missing keys keep the stage's value; an empty map is the stage itself
    for stage in (1, 2):
        assert YOLONet(training=True, plan_only=True, stage=stage, lock={}).lock == \
            YOLONet(training=True, plan_only=True, stage=stage).lock == O.default_lock(stage)
    assert YOLONet(training=True, plan_only=True, stage=2, lock={5: True}).pass_through_layers() == [5]


@pytest.mark.parametrize("key,m", [(0, 2), (83, 2), (-1, 2), (80, 4), (86, 1), ("5", 2), (5.0, 2)])
def test_lock_key_outside_the_net_is_a_value_error(key, m):
    with pytest.raises(ValueError, match="lock"):
        YOLONet(training=True, plan_only=True, mask_stride=m, lock={key: True})


def test_last_layer_of_every_mask_stride_is_a_valid_key():
    for m, last in ((4, 79), (2, 82), (1, 85)):
        net = YOLONet(training=True, plan_only=True, stage=2, mask_stride=m, lock={last: True})
        assert net.lock[last] and net.pass_through_layers() == [last]


@pytest.mark.parametrize("name", sorted(MAPS))
def test_holed_map_variables_arena_and_pass_through_set(name):
    net, m, lock = _net(name)
    assert net.lock == lock
    if m == 2:
        shapes = {n: tuple(t.shape) for n, t in O.init_params(lock=O.default_lock(2)).items()}
        trainable, reg = O.trainable_names(lock), O.regularized_names(lock)
    else:
        shapes = R.variable_shapes(m, net.k)
        lay = lambda n: int(n.split("convolutional")[1].split("/")[0])
        trainable = [n for n in shapes if not lock[lay(n)] and not n.split("/")[-1].startswith("moving_")]
        reg = R.regularized_names(shapes, lock)
    assert set(net.trainable_names()) == set(trainable) and len(net.trainable_names()) == len(trainable)
    numel = lambda n: int(torch.Size(shapes[n]).numel())
    assert net.n_decay == sum(numel(n) for n in reg)
    assert net.n_params == sum(numel(n) for n in trainable)
    # the arena: [weights (+ biases) in layer order | gamma, beta in layer order], no gap, no overlap
    spans = sorted(net.arena_slices.values())
    assert spans[0][0] == 0 and spans[-1][0] + spans[-1][1] == net.n_params
    assert all(a[0] + a[1] == b[0] for a, b in zip(spans, spans[1:]))
    w_spans = [net.arena_slices["yolo/convolutional%d/weights" % l.idx] for l in net.layers if not l.lock]
    assert [o for o, _ in w_spans] == sorted(o for o, _ in w_spans) and all(o + c <= net.n_decay for o, c in w_spans)
    net._plan_opt_chunks()          # (asserts contiguity of the regularised region in layer order itself)
    assert set().union(*[ch["members"] for ch in net.opt_chunks]) == {l.idx for l in net.layers if not l.lock}
    # pass-through layers: an independent walk of the reference's graph
    assert net.pass_through_layers() == pass_through(m, lock)
    assert net.pass_through_layers(), "every map of this file has a hole"
    for l in net.layers:
        assert not (l.passthru and not l.lock)


def test_pass_through_sets_spelled_out():
    """the package's sets against sets read off the graph by hand (and the test's own walk against the same)"""
    want = {"hole_5_9": [5, 6, 7, 8, 9], "frozen_heads": list(range(53, 76)),
            "stage1_hole": [62, 63, 64],                       # conv1-52: nothing trainable upstream
            "m1_hole": [83, 84], "odd": list(range(3, 83, 2))}  # conv1 reads the image only
    for name, layers in want.items():
        m, lock = lock_of(name)
        assert YOLONet(training=True, plan_only=True, mask_stride=m, lock=lock).pass_through_layers() == layers, name
        assert pass_through(m, lock) == layers, name
    assert YOLONet(training=True, plan_only=True, lock={i: i <= 75 for i in range(1, 83)}).pass_through_layers() == []


def test_reference_stages_and_inference_nets_have_no_pass_through_layer():
    for stage in (1, 2):
        assert YOLONet(training=True, plan_only=True, stage=stage).pass_through_layers() == []
    m, lock = lock_of("hole_5_9")
    assert YOLONet(training=False, plan_only=True, lock=lock).pass_through_layers() == []


def test_layer_roles_equal_the_spelled_out_predicates_and_the_gradients_way():
    """the role slots (trains, train_bn, keeps_raw, on_path) against the predicates they replaced, and on_path against an
    independent walk of the reference's graph: exactly the layers with a trainable layer at or upstream of them and a loss
    downstream.  Every lock map of lock_maps.py and both stages at every mask stride, training and not.  On the layer table,
    through the function the constructor itself calls (YOLONet._mark_pass_through): a plan-only net takes seconds to
    initialise its variables, and its roles are a function of (table, lock map, training) alone"""
    cases = [(lock_of(name)) for name in list(MAPS) + list(STRIDE_MAPS)]
    cases += [(m, {i: (stage == 1 and i <= 52) for i in range(1, SCORE_LAYER[m] + 1)}) for stage in (1, 2) for m in (1, 2, 4)]
    for m, lock in cases:
        ins = inputs_of(m)
        readers = {i: [j for j in ins if i in ins[j]] for i in ins}
        losses = {59, 67, 75, SCORE_LAYER[m]}

        def above(i, seen):          # i and everything upstream of it
            if i and i not in seen:
                seen.add(i)
                for j in ins[i]:
                    above(j, seen)
            return seen

        def reaches_loss(i):
            return i in losses or any(reaches_loss(j) for j in readers[i])

        for training in (True, False):
            layers = build_topology(80, 3, m)
            YOLONet._mark_pass_through(layers, lock, training)
            assert [l.idx for l in layers] == sorted(ins)
            for l in layers:
                what = "m = %d, layer %d, training %s" % (m, l.idx, training)
                assert l.lock == lock[l.idx], what
                assert l.trains == (training and not l.lock), what
                assert l.train_bn == (training and (not l.lock) and l.kind != "lin"), what
                assert l.keeps_raw == (training and (not l.lock or l.passthru) and l.kind != "lin"), what
                assert l.on_path == (training and (not l.lock or l.passthru)), what
                assert (not l.on_path) == (not training or (l.lock and not l.passthru)), what
                assert (l.on_path or (training and l.kind == "lin")) == \
                    (training and (not l.lock or l.passthru or l.kind == "lin")), what
                assert all(isinstance(v, bool) for v in (l.trains, l.train_bn, l.keeps_raw, l.on_path, l.passthru)), what
                want = training and any(not lock[t] for t in above(l.idx, set())) and reaches_loss(l.idx)
                assert l.on_path == want, what
            assert [l.idx for l in layers if l.passthru] == (pass_through(m, lock) if training else [])


def test_a_plan_only_net_carries_the_roles_of_its_table():
    m, lock = lock_of("stage1_hole")
    net = YOLONet(training=True, plan_only=True, mask_stride=m, lock=lock)
    layers = build_topology(net.num_class, net.k, m)
    assert YOLONet._mark_pass_through(layers, lock, True) == net._needs_grad_into
    for a, b in zip(net.layers, layers):
        assert (a.lock, a.passthru, a.trains, a.train_bn, a.keeps_raw, a.on_path) == \
            (b.lock, b.passthru, b.trains, b.train_bn, b.keeps_raw, b.on_path)
    assert [l.idx for l in net.layers if l.on_path] == list(range(53, 83))


def test_fp8_refuses_a_lock_map_that_breaks_the_fp8_chain():
    # conv10-30 would run fp8, conv31 trains: no mixed chain
    with pytest.raises(ValueError, match="layer 31 is trainable"):
        YOLONet(training=True, plan_only=True, dtype="fp8", lock={i: i <= 30 for i in range(1, 83)})
    # conv20 trains, conv21.. are locked behind it (pass-through); the chain breaks at 20
    with pytest.raises(ValueError, match="layer 20"):
        YOLONet(training=True, plan_only=True, dtype="fp8", stage=1, lock={20: False})
    # a hole BEHIND conv52 leaves the fp8 prefix whole
    m, lock = lock_of("stage1_hole")
    net = YOLONet(training=True, plan_only=True, dtype="fp8", lock=lock)
    assert [l.idx for l in net._fp8_layers()] == list(range(net.FP8_FROM, 53))
    # an inference net never trains: any map
    m, lock = lock_of("hole_5_9")
    net = YOLONet(training=False, plan_only=True, dtype="fp8", lock=lock)
    assert [l.idx for l in net._fp8_layers()] == list(range(net.FP8_FROM, 53))


def test_data_parallel_buckets_cover_a_holed_arena(tmp_path):
    """dp.py plans its buckets over the trainable spans: one gloo rank, a holed map, the real protocol"""
    import torch.distributed as dist
    from disyolo_amd.dp import enable_data_parallel
    os.environ.setdefault("GLOO_SOCKET_IFNAME", "lo")
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    try:
        for name in ("hole_5_9", "stage1_hole", "odd"):
            net, m, lock = _net(name, seed=3)
            dp = enable_data_parallel(net, bucket_mb=4.0)
            covered = sorted((o, o + c) for _, o, c in dp.buckets)
            assert covered[0][0] == 0 and covered[-1][1] == net.n_decay
            assert all(a[1] == b[0] for a, b in zip(covered, covered[1:]))
            assert set().union(*dp.members) == {l.idx for l in net.layers if not l.lock}
            g = torch.randn(net.n_params, generator=torch.Generator().manual_seed(5))
            net.grad_arena.copy_(g)
            fired = 0
            dp.begin_step()
            for l in net.backward_order():
                if l.lock:
                    continue                        # (backward() hands only trainable layers to on_layer_done)
                before = len(dp.works)
                dp.on_layer_done(l)
                fired += len(dp.works) > before
            dp.finish()
            assert fired == len(dp.buckets)
            assert torch.equal(net.grad_arena, g)   # one rank: the sum is the gradient itself
    finally:
        dist.destroy_process_group()
