"""The whole update step under a pairwise covering array of the kernel-selection knobs (tests/knob_matrix_helpers.py):
every (base net, row) is one case.  The knobs are set before the net is created and restored in a ``finally``.

Per case, on a net whose gradient buffer and workspace start as NaN:
 (a) one applied step against the base's float64 reference at the zoo's bars (``net_zoo_helpers.BARS``, ``assert_update_close``),
     every gradient element finite -- the bars do not move with the row: all knob forms compute the same arithmetic up to
     fp32 summation order.  (No seed gives the 255-frame base's reference the zoo's margins; it is held to the same bars with the
     margins ``knob_matrix_helpers.B255`` states.)
 (b) the reported plan equals the words predicted from the step's conditions, and every capacity is respected;
 (c) the same step with ``fwd_fuse12_flat`` flipped, and with ``bwd_dense_lean`` flipped, gives the loss, every gradient and
     the post-step parameters bit for bit, whether the row's knobs put the fused forms inside or outside their envelopes;
 (d) the same step again from the restored parameters, on the workspace the first left, is the first bit for bit, report
     included;
 (e) 33-frame PPO bases: a second consecutive step without restoring, against the float64 oracle evaluated at the
     parameters read back after step 1, its Adam state advanced likewise: the step from a used workspace, moments and step
     count.  (A single-step call joins the side stream's share of its update before it returns, so this does NOT show a
     forward that reads weights too early: (f) does.)  Where that reference has a relu unit within RELU_MARGIN of its kink the
     case skips (e) alone and says so; at most ``MAX_SECOND_SKIPS`` cases of a base may -- counted per process, in
     collection order: a run split over several processes counts per process;
 (f) cnn84_h512_a4_b33 (``ppo_train``: 80 rows, batch 33, two epochs: minibatches of 33, 33 and 14) and impala84_a4_t9x3
     (``impala_train``: three chunks of 27 frames): the eager, the capturing and the replayed train AND a chain of single-step
     calls over the same minibatches end in the same parameters bit for bit.  The trains leave the side stream's Adam share
     (tail_overlap bit 2) pending into the next step's forward, the chain never does: a join in the wrong place differs.
     One capture per train.
Each case prints one ``KNOB`` JSON line.  Measured figures: profiles/knob_matrix_parity.md."""
import json
import time
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

import knob_matrix_helpers as K
import net_zoo_helpers as Z
from test_gpu_learner import assert_update_close
from test_gpu_net_zoo import WS_ARMED_TAIL, _check_capacities, _device_inputs, _run, _up

pytestmark = pytest.mark.gpu

CASES = [(bid, ri) for bid in K.BASES for ri in range(len(K.array()))]
_SECOND_SKIPS = {bid: [] for bid in K.BASES}


def _parity(rid, ref_out, init, loss, grads, weights, gnorm, tag, bars):
    """(a) / (e): loss, every gradient tensor, the gradient norm and the update against ``ref_out`` at the zoo's bars ->
    the errors as fractions of them"""
    loss_e = abs(loss - float(ref_out["loss"])) / max(1.0, abs(float(ref_out["loss"])))
    worst, worst_k = 0.0, None
    for k, r in ref_out["grads"].items():
        g = grads[k].reshape(r.shape)
        assert np.any(r), (rid, tag, k)
        e = Z.rel_err(g, r)
        if e > worst:
            worst, worst_k = e, k
    gn_e = None
    if ref_out["gnorm"] is not None:
        gn_e = abs(gnorm - float(ref_out["gnorm"])) / float(ref_out["gnorm"])
    frac = dict(loss=loss_e / bars["loss"], grad=worst / bars["grad"], grad_k=worst_k,
                gnorm=None if gn_e is None else gn_e / bars["gnorm"])
    print("KNOB-{} {}".format(tag, json.dumps(dict(id=rid, **frac))))
    assert loss_e <= bars["loss"], (rid, tag, loss, float(ref_out["loss"]))
    assert worst < bars["grad"], (rid, tag, worst_k, worst)
    if gn_e is not None:
        assert gn_e < bars["gnorm"], (rid, tag, gnorm, float(ref_out["gnorm"]))
    assert_update_close({k: weights[k] for k in ref_out["params"]}, ref_out["params"], init, ref_out["lr"], rid + tag)
    return frac


def _capacities(rep, spec, b):
    """``test_gpu_net_zoo._check_capacities``, whose first assertion also holds an UNSPLIT layer's output against the split-K
    partial buffer.  Such a layer never touches that buffer (``launch_fwd`` writes its output in place when ksplit == 1), and
    the zoo's batches of at most 33 frames never exceed it, but the 255-frame first layer does (102 000 x 32 floats).  So the
    split layers are held against the real capacity here, and the zoo's check then sees a buffer that holds the unsplit
    outputs as well: on the 33-frame bases that is the buffer's own size, the zoo's check unchanged."""
    m = [b * lay.OH * lay.OW * lay.N for lay in spec.layers]
    for li, l in enumerate(rep["layer"]):
        assert l["ksplit"] >= 1 and (l["ksplit"] == 1 or l["ksplit"] * m[li] <= rep["partial_floats"]), (li, l)
    unsplit = [m[li] for li, l in enumerate(rep["layer"]) if l["ksplit"] == 1]
    _check_capacities(dict(rep, partial_floats=max([rep["partial_floats"]] + unsplit)), spec, b)


def _train_check(net, spec, params, base):
    """(f) the base's train entry over three minibatches / chunks per pass: eager, capturing and replayed, and the same
    updates as a chain of single-step calls -> [(loss sum, flat parameters)] of the four runs, and the captures each train added.
    The trains defer the join of the side stream's Adam share (tail_overlap bit 2) into the NEXT step's forward; a single-step
    call joins before it returns, so the chain's result does not depend on where the forward joins."""
    from xingtian_amd import lib as L
    row = base["row"]
    if base["train"] == "ppo":
        # 80 rows, batch 33, two epochs: minibatches of 33, 33 and 14 (the shapes of
        # test_gpu_fwd_fuse12_flat.py::test_train_graph_replay_against_eager_and_switch_off)
        from test_gpu_learner import synth_ppo_rollout
        cfg = dict(Z.PPO_CFG, BATCH_SIZE=33, NUM_SGD_ITER=2)
        rng = np.random.default_rng(3)
        n, steps = 80, 6
        obs, lab = synth_ppo_rollout(rng, n, (84, 84, 4), 4)
        perms = _up(np.stack([rng.permutation(n) for _ in range(2)]).astype(np.int32))
        data = [_up(lab[0])] + [_up(x.reshape(-1)) for x in lab[1:]]
        dobs, c = net.to_device_obs(obs), net.make_ppo_cfg(cfg)

        def train(use_graph):
            return net.ppo_train(c, dobs, perms, *data, use_graph=use_graph)

        def chain():
            for ep in range(2):
                for lo in range(0, n, 33):
                    net.ppo_step(c, dobs, perms[ep, lo:min(lo + 33, n)], *data, apply=True)
    else:
        # three chunks of the base's own 27 frames (3 trajectories of 9 steps each)
        t_len, ntraj = row["batch"]
        inp = Z.make_inputs(dict(row, batch=(t_len, 3 * ntraj), seed=row["seed"] + 100))
        n, chunk, steps = 3 * t_len * ntraj, t_len * ntraj, 3
        dobs, c = net.to_device_obs(inp["obs"]), net.make_impala_cfg(Z.IMPALA_LR, Z.IMPALA_CLIP, t_len)
        data = [_up(inp["bp"]), _up(inp["action"]), _up(inp["done"].astype(np.uint8)), _up(inp["reward"])]

        def train(use_graph):
            return net.impala_train(c, dobs, chunk, *data, use_graph=use_graph)

        def chain():
            for lo in range(0, n, chunk):
                net.impala_step(c, dobs[lo:lo + chunk], *[x[lo:lo + chunk] for x in data], apply=True)

    out, captures = [], []
    for how in (False, True, True, "chain"):
        net.set_weights({k: v.reshape(spec.names[k][1]) for k, v in params.items()})
        net.reset_optimizer()
        before = L.graph_cache_info(net.handle)["captures"]
        loss = None
        if how == "chain":
            chain()
        else:
            acc = train(how)
        torch.cuda.synchronize()
        if how != "chain":
            a = acc.cpu().numpy()
            assert a[1] == float(steps), a
            loss = float(a[0])
        assert all(np.isfinite(w).all() for w in net.get_weights().values())
        out.append((loss, np.nan_to_num(net.params.detach().cpu().numpy(), nan=0.0)))      # (the buffer's padding is NaN)
        captures.append(L.graph_cache_info(net.handle)["captures"] - before)
    return out, captures


# check (b), FINISH_FORM under tail_fused: the fused tail runs where its grid is resident at once, and that capacity is ONE
# number per device.  [largest grid seen fused, smallest grid seen unfused] of this process
_FUSED_GRIDS = [0, 1 << 30]


@pytest.mark.parametrize("bid,ri", CASES, ids=["{}-r{:02d}".format(b, r) for b, r in CASES])
def test_step_under_the_row_of_knobs(bid, ri):
    from xingtian_amd import lib as L
    from xingtian_amd.model.hip_net import HipActorCritic
    t0 = time.perf_counter()
    base, knobs = K.BASES[bid], K.array()[ri]
    row = base["row"]
    rid = "{}-r{:02d}".format(bid, ri)
    spec, ospec, params0, inp = K.build(row)
    ref, bars = Z.reference(row), base["bars"]
    b = Z.frames(row)
    want = K.expected_words(row, spec, knobs)
    env_open = K.conv12_envelope_open(spec, b, knobs)
    old = L.set_tuning(**K.tuning_of(knobs))
    old_lean = L.set_bwd_dense_lean(bool(knobs["bwd_dense_lean"]))
    flips, second, graph = OrderedDict(), None, None
    try:
        net = HipActorCritic(spec, max_batch=b, seed=0)
        net.set_fwd_fuse12_flat(bool(knobs["fwd_fuse12_flat"]))
        net.set_weights({k: v.reshape(spec.names[k][1]) for k, v in params0.items()})
        dev = _device_inputs(row, net, inp)
        net.grads.fill_(float("nan"))
        net.workspace[:net.workspace.numel() - WS_ARMED_TAIL].fill_(float("nan"))
        torch.cuda.synchronize()
        tensors = (net.params, net.adam_m, net.adam_v, net.adam_state)
        saved = [x.clone() for x in tensors]
        w_init = net.get_weights()

        def restore():
            for dst, src in zip(tensors, saved):
                dst.copy_(src)
            net.touch()

        def step():
            loss = _run(row, net, None, dev)
            return dict(loss=loss, rep=net.last_step_report(), g=net.grads.clone(), p=net.params.clone(),
                        state=net.adam_state.cpu().numpy().copy())

        s1 = step()
        grads, weights = net.grads_dict(), net.get_weights()

        # (c) each bit-preserving switch flipped against the row's own setting
        restore()
        net.set_fwd_fuse12_flat(not knobs["fwd_fuse12_flat"])
        flips["fwd_fuse12_flat"] = step()
        net.set_fwd_fuse12_flat(bool(knobs["fwd_fuse12_flat"]))
        restore()
        L.set_bwd_dense_lean(not knobs["bwd_dense_lean"])
        flips["bwd_dense_lean"] = step()
        L.set_bwd_dense_lean(bool(knobs["bwd_dense_lean"]))

        # (d) the same step again, on the workspace the steps before left
        restore()
        s2 = step()

        # (e) a second consecutive step: the net is where step 1 left it
        if base["second"]:
            after1 = {k: np.array(weights[k], copy=True).reshape(v.shape) for k, v in params0.items()}
            s3 = step()
            second = dict(s=s3, grads=net.grads_dict(), weights=net.get_weights(), after1=after1)

        # (f) eager, captured and replayed trains under the row's knobs
        if base["train"]:
            graph = _train_check(net, spec, params0, base)
    finally:
        L.set_bwd_dense_lean(old_lean)
        L.set_tuning(**old)

    rep = s1["rep"]
    got = K.report_words(rep)
    line = OrderedDict(id=rid, base=bid, row=ri, knobs=K.non_default(knobs), envelope_open=env_open, conv12=want["conv12"],
                       plan={k: got[k] for k in ("tail_overlap", "finish_form", "fwd_fuse12", "bwd_fuse21", "ksplit", "deferred",
                                                 "mask_valid")},
                       msplit=[l["msplit"] for l in rep["layer"]], blocks=rep["finish_blocks"],
                       # (informational: which tensors' bits a row changes against row 0, profiles/knob_matrix_parity.md)
                       bits=OrderedDict([("loss", float(s1["loss"]).hex())] +
                                        [(k, "{:08x}".format(zlib.crc32(np.ascontiguousarray(g).tobytes()))) for k, g in grads.items()]))

    # every gradient element was written
    for k, g in grads.items():
        assert np.isfinite(g).all(), (rid, k, "an element of the gradient is not finite")
    assert all(np.isfinite(w).all() for w in weights.values()), rid

    # (a) parity with the float64 reference
    frac = _parity(rid, ref["out"], {k: w_init[k] for k in ref["out"]["params"]}, s1["loss"], grads, weights,
                   float(s1["state"][4]), "a", bars)
    line.update(loss=frac["loss"], grad=frac["grad"], grad_k=frac["grad_k"], gnorm=frac["gnorm"], grad_bar=bars["grad"])

    # (c), (d) bit for bit
    eq = lambda x, y: torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0))
    for name, s in flips.items():
        bad = [w for w, same in (("loss", s["loss"] == s1["loss"]), ("grads", eq(s["g"], s1["g"])),
                                 ("params", eq(s["p"], s1["p"])), ("state", np.array_equal(s["state"], s1["state"]))) if not same]
        assert not bad, (rid, name + " flipped changes bits of", bad, "envelope open" if env_open else "envelope closed")
    assert s2["loss"] == s1["loss"] and s2["rep"] == rep and eq(s2["g"], s1["g"]) and eq(s2["p"], s1["p"]) and \
        np.array_equal(s2["state"], s1["state"]), (rid, "the repeated step differs")

    # (b) the plan
    form_ok = want["finish_form"]
    diff = {k: (want[k], got[k]) for k in got if k != "finish_form" and want[k] != got[k]}
    assert not diff and got["finish_form"] in form_ok, (rid, diff, got["finish_form"], form_ok)
    if len(form_ok) > 1:      # tail_fused asked for: fused (3) wherever the grid is resident, see _FUSED_GRIDS
        nslab = [l["msplit"] for l in rep["layer"]] + [rep["head_chunks"]] * 2
        grid = K.fused_grid(K.grad_counts(spec), nslab, knobs)
        line["fused_grid"] = grid
        if got["finish_form"] == 3:
            assert grid <= 2048, (rid, grid)      # (what any device of this kind can hold)
            _FUSED_GRIDS[0] = max(_FUSED_GRIDS[0], grid)
        else:
            _FUSED_GRIDS[1] = min(_FUSED_GRIDS[1], grid)
            # one workgroup of 256 threads per CU is resident whatever the kernel's registers: such a grid is never refused
            assert grid > torch.cuda.get_device_properties(0).multi_processor_count, (rid, grid)
        assert _FUSED_GRIDS[0] < _FUSED_GRIDS[1], (rid, "a smaller grid ran unfused than one that ran fused", _FUSED_GRIDS)
    _capacities(rep, spec, b)

    # (e)
    if second is not None:
        first = K.first_step_state(row)
        _, out2 = K.ppo_oracle_at(row, ospec, second["after1"], inp, steps_before=1, m=first["m"], v=first["v"])
        line["second_min_relu_z"] = out2["min_relu_z"]
        if out2["min_relu_z"] < Z.RELU_MARGIN:
            _SECOND_SKIPS[bid].append(ri)
            line["second"] = "skipped"
            print("KNOB-e {} skips the second step: min_relu_preact {:.2e} of the read-back parameters' reference".format(
                rid, out2["min_relu_z"]))
            assert len(_SECOND_SKIPS[bid]) <= K.MAX_SECOND_SKIPS, (bid, _SECOND_SKIPS[bid])
        else:
            s3 = second["s"]
            for k, g in second["grads"].items():
                assert np.isfinite(g).all(), (rid, k, "second step")
            frac = _parity(rid, out2, second["after1"], s3["loss"], second["grads"], second["weights"], float(s3["state"][4]), "e", bars)
            line.update(loss2=frac["loss"], grad2=frac["grad"], grad2_k=frac["grad_k"], gnorm2=frac["gnorm"])
            assert s3["rep"] == rep, (rid, "the second step reports another plan")

    # (f)
    if graph is not None:
        out, captures = graph
        for which, o in zip(("captured", "replayed", "chain of single steps"), out[1:]):
            assert which.startswith("chain") or o[0] == out[0][0], (rid, which + " train: another loss than the eager one")
            assert np.array_equal(o[1], out[0][1]), (rid, which + ": other parameters than the eager train")
        # One train is ONE cached graph (its key holds n and the batch size; the minibatches are nodes of it): captured once,
        # replayed from the cache.  The key holds no tuning word -- "set the knobs before creating networks" -- so this counts
        # the row's own capture only because every case creates its net after setting the knobs.
        assert captures == [0, 1, 0, 0], (rid, captures)
        line["graph_captures"] = captures

    line["seconds"] = round(time.perf_counter() - t0, 2)
    print("KNOB " + json.dumps(line))
