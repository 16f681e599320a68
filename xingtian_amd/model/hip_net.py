"""Device-resident actor-critic network driven through the C ABI.

PyTorch-ROCm tensors are storage only (flat parameter / gradient / Adam buffers, the
activation workspace, the resident rollout); every arithmetic op is a HIP kernel in
``libxt_mi355x.so``.  Used by the ``PPO`` / ``ImpalaCnnOpt`` model classes.
"""
import ctypes
from collections import OrderedDict

import numpy as np
import torch

from xingtian_amd import lib as L
from xingtian_amd.model.cpu_net import initial_weights


def keras_lr_t(lr, iterations, decay=0.0, beta1=0.9, beta2=0.999):
    """Step size of tf.keras Adam's update number ``iterations + 1``: the time-decayed learning rate times the bias
    correction, in float32 as the optimizer's graph computes it (what ``xt_adam_keras`` takes as ``lr_t``)."""
    t = iterations + 1
    lr_t = np.float32(lr) / (np.float32(1.0) + np.float32(decay) * np.float32(iterations))
    return lr_t * np.sqrt(np.float32(1.0) - np.float32(beta2) ** t) / (np.float32(1.0) - np.float32(beta1) ** t)


def keras_fit_table(n_rows, batch_size, fit_batch, iterations, lr, decay):
    """The minibatches of one ``IMPALA.train`` over ``n_rows`` transitions, in execution order: the algorithm calls
    ``model.fit`` once per sequential ``batch_size`` chunk, a fit walks its chunk in minibatches of ``fit_batch`` and
    every minibatch is one Adam update.  -> [(offset into the concatenated per-chunk orders, rows, chunk number,
    lr_t)], ``lr_t`` = ``keras_lr_t`` at ``iterations`` + the number of updates before this one."""
    table = []
    for chunk, lo in enumerate(range(0, n_rows, batch_size)):
        n = min(batch_size, n_rows - lo)
        for m in range(0, n, fit_batch):
            table.append((lo + m, min(fit_batch, n - m), chunk, float(keras_lr_t(lr, iterations + len(table), decay))))
    return table


class _MailboxDone(object):
    """see ``HipActorCritic.io_publish_done``"""
    __slots__ = ("net", "seq")

    def __init__(self, net, seq):
        self.net, self.seq = net, seq

    def synchronize(self):
        rc = self.net.lib.xt_net_io_publish_wait(self.net.handle, self.seq, 30000)        # (ctypes releases the GIL)
        if rc == 1:
            raise RuntimeError("xingtian_amd: the parameter copy of train {} did not land within 30 s".format(self.seq))
        L.check(rc, "xt_net_io_publish_wait")

    def query(self):
        return self.net.lib.xt_net_io_publish_wait(self.net.handle, self.seq, 0) == 0


def net_desc(spec):
    """``NetSpec`` -> (layer array, ``NetDesc``) of the C ABI; the array must outlive the description"""
    lay_arr = (L.LayerDesc * len(spec.layers))()
    for i, lay in enumerate(spec.layers):
        g = lay_arr[i].g
        g.H, g.W, g.C, g.KH, g.KW, g.S = lay.H, lay.W, lay.C, lay.KH, lay.KW, lay.S
        g.PT, g.PL, g.OH, g.OW, g.N, g.act = lay.PT, lay.PL, lay.OH, lay.OW, lay.N, L.ACT[lay.act]
        lay_arr[i].param_off = lay.param_off
        lay_arr[i].trunk = lay.trunk
    d = L.NetDesc()
    d.n_layers, d.layers, d.n_trunks = len(spec.layers), lay_arr, spec.n_trunks
    # (a noisy spec: the net sees the n_net floats of the effective parameters; the store behind them is the learner's)
    d.feat, d.action_dim, d.pi_off, d.v_off = spec.feat, spec.action_dim, spec.pi_off, spec.v_off
    d.n_params = getattr(spec, "n_net", spec.n_flat)
    d.xf = L.InputXform(*spec.input_xform)
    d.in_h, d.in_w, d.in_c = spec.layers[0].H, spec.layers[0].W, spec.layers[0].C      # (C: as the kernels read it, padded)
    d.action_type = L.ACTION_TYPE[getattr(spec, "action_type", "Categorical")]
    d.logstd_off = getattr(spec, "logstd_off", 0)
    return lay_arr, d


def create_net(spec, max_batch):
    """C ABI ``xt_net_create`` (host code, no device call) -> (layer array, description, handle).  A network outside the
    library's envelope -- more than ``lib.MAX_TRUNK_LAYERS`` trunk layers, an empty layer, unequal unshared
    trunks -- is a ``ValueError`` carrying the library's message, raised before anything is allocated or enqueued."""
    lib = L.load()
    lay_arr, d = net_desc(spec)
    h = ctypes.c_void_p()
    rc = lib.xt_net_create(ctypes.byref(d), int(max_batch), ctypes.byref(h))
    if rc != 0:
        msg = lib.xt_last_error()
        raise ValueError("xingtian_amd: this network cannot be built (xt_net_create, rc={}): {}".format(
            rc, msg.decode() if msg else "?"))
    return lay_arr, d, h


class HipActorCritic(object):
    def __init__(self, spec, max_batch, device="cuda:0", seed=None, init="glorot"):
        self.lib = L.load()
        self.spec, self.max_batch = spec, int(max_batch)
        # host code only: a description the library cannot serve is a ValueError here, with or without a GPU
        self._lay_arr, self._desc, self.handle = create_net(spec, self.max_batch)
        h = self.handle
        L.require_gpu()
        self.device = torch.device(device)
        torch.cuda.set_device(self.device)
        n = spec.n_flat
        self.params = torch.zeros(n, dtype=torch.float32, device=self.device)
        # the gradient buffer carries XT_DP_TAIL_FLOATS behind align4(n): the data-parallel tail (rows / loss share of every
        # rank, include/xt_mi355x.h `xt_net_set_dp`) travels with the gradient in ONE exchange; `grads` is the gradient view
        self.grads_xchg = torch.zeros(((n + 3) // 4) * 4 + L.DP_TAIL_FLOATS, dtype=torch.float32, device=self.device)
        self.grads = self.grads_xchg[:n]
        self.adam_m = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.adam_v = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.adam_state = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.loss_acc = torch.zeros(8, dtype=torch.float32, device=self.device)
        self.loss_out = torch.zeros(8, dtype=torch.float32, device=self.device)

        ws_bytes = self.lib.xt_net_workspace_bytes(h)
        self.workspace = torch.empty(ws_bytes // 4, dtype=torch.float32, device=self.device)
        # a noisy spec (netspec._add_noisy): ``params`` / ``grads`` / the Adam slots are the STORE (means in the net's layout,
        # the sigma blocks behind n_net) and the net is bound to ``params_eff``, the n_net effective parameters ``compose``
        # writes; the backward leaves g_mu in grads[0, n_net).  A plain spec allocates nothing more.
        self.params_eff = self.noise = None
        if getattr(spec, "noisy_layers", None):
            self.params_eff = torch.zeros(spec.n_net, dtype=torch.float32, device=self.device)
            self.noise = torch.zeros(spec.noise_floats, dtype=torch.float32, device=self.device)
            self._noisy_table = (L.NoisyLayer * len(spec.noisy_layers))(*[
                L.NoisyLayer(nl.w_off, nl.sigma_off, nl.noise_off, nl.K, nl.N, nl.index, 0) for nl in spec.noisy_layers])
        bound = self.params if self.params_eff is None else self.params_eff
        L.check(self.lib.xt_net_bind(h, L.ptr(bound), L.ptr(self.grads), L.ptr(self.adam_m), L.ptr(self.adam_v),
                                     L.ptr(self.adam_state), L.ptr(self.workspace), ws_bytes), "xt_net_bind")
        L.check(self.lib.xt_adam_state_init(L.ptr(self.adam_state), L.stream_ptr()), "xt_adam_state_init")
        if init == "glorot":
            self.init_weights(seed)

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.xt_net_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    inference_only = False

    def init_weights(self, seed=None, baseline_norm_std=None):
        self.set_weights(initial_weights(self.spec, seed, baseline_norm_std))

    def _flat_to_host(self, dev_flat, tag):
        """One D2H of a flat device buffer into a persistent PINNED host buffer (the weight publish
        after every PPO update is on the critical path; a pageable .cpu() bounces through a driver staging copy)."""
        pin = getattr(self, "_pin", None)
        if pin is None:
            pin = self._pin = {}
        if tag not in pin:
            pin[tag] = torch.empty(dev_flat.shape, dtype=dev_flat.dtype, pin_memory=True)
        pin[tag].copy_(dev_flat.detach(), non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return pin[tag].numpy()

    # ---- weight publish: the D2H of the new parameters is enqueued by the update itself
    SNAP_SLOTS = 4

    def touch(self):
        """The parameters are about to change (or have been assigned): a snapshot taken earlier is stale."""
        self._version = getattr(self, "_version", 0) + 1

    def snapshot_weights_async(self):
        """Enqueue the D2H of the flat parameter buffer into the next of ``SNAP_SLOTS`` pinned host blocks on a side
        stream, ordered after everything already enqueued on the compute stream (the update whose result it
        publishes).  Returns immediately: the copy runs under whatever the host does next (the loss read-back, the next
        rollout's ingest).  ``get_weights`` picks the block up once its event has fired."""
        ring = getattr(self, "_wring", None)
        if ring is not None and not getattr(ring, "pinned", False):
            ring = self._wring = None       # the ring was closed (or un-pinned) behind our back: private snapshots again
        if ring is not None and getattr(ring, "async_commit", False):
            # asynchronous commit (WeightsRing.start_committer): every begun copy IS a publish; the ring's helper thread makes
            # it visible when it lands (begin blocks only when slots - 1 copies are still in flight)
            ring.begin_flat_publish(self, getattr(self, "_wring_ctr", None))
            self._wring_version = getattr(self, "_version", 0)
            return
        if ring is not None:
            # a page-locked WeightsRing is attached: the copy goes straight into its next slot (no pinned bounce block).
            # Begun publishes beyond the allowed lag belong to updates whose weights were never handed out: reuse their slot
            while len(ring._pending) > getattr(self, "_wring_lag", 0):
                ring.retarget_flat_publish()
            ring.begin_flat_publish(self, getattr(self, "_wring_ctr", None))
            self._wring_version = getattr(self, "_version", 0)
            return
        snap = getattr(self, "_snap", None)
        if snap is None:
            snap = self._snap = dict(stream=torch.cuda.Stream(device=self.device), slot=-1, version=-1, events=[],
                                     host=[torch.empty(self.params.shape, dtype=torch.float32, pin_memory=True)
                                           for _ in range(self.SNAP_SLOTS)])
            snap["events"] = [torch.cuda.Event() for _ in range(self.SNAP_SLOTS)]
            snap["ready"] = [torch.cuda.Event() for _ in range(self.SNAP_SLOTS)]
        i = (snap["slot"] + 1) % self.SNAP_SLOTS
        ready = snap["ready"][i]
        ready.record(L.current_stream(self.device))
        snap["stream"].wait_event(ready)
        L.memcpy_async(snap["host"][i].data_ptr(), self.params.data_ptr(), self.params.numel() * 4, L.D2H, snap["stream"])
        snap["events"][i].record(snap["stream"])
        snap["slot"], snap["version"] = i, getattr(self, "_version", 0)

    def get_weights(self, copy=True):
        """dict TF-variable-name -> ndarray (TFVariables.get_weights, xt/model/tf_utils.py:99-102).  The flat
        parameter buffer IS the packed form: ONE pinned D2H -- already in flight when the last update enqueued it
        (``snapshot_weights_async``), else issued now.  By default the arrays are private copies, as the reference hands
        them out (a caller may keep them: best-checkpoint retention, PBT).  ``copy=False`` returns per-variable VIEWS into
        the pinned block, valid until ``SNAP_SLOTS - 1`` further snapshots have been taken: for consumers that
        serialise them at once (``transport.WeightsRing.publish``, ``save_model``)."""
        flat = self._snapshot_flat()
        if copy:
            # ONE private block per call (the native staging pool moves the 3.4 MB at ~100 GB/s instead of a dozen
            # single-threaded numpy copies: 0.24 -> ~0.1 ms per publish); the dict's arrays are views of that block, which
            # nobody else holds
            own = np.empty(flat.shape, np.float32)
            if not getattr(self, "_tuned_copy", False):
                from xingtian_amd.ingest import staging_report
                staging_report()
                self._tuned_copy = True
            L.check(self.lib.xt_stage_rows(ctypes.c_void_p(own.ctypes.data), ctypes.c_void_p(flat.ctypes.data), own.nbytes,
                                           None, 0, 0, -1, None), "xt_stage_rows")
            flat = own
        out = OrderedDict()
        for name in self.spec.names:
            out[name] = self.spec.var_view(flat, name)
        return out

    def _snapshot_flat(self):
        """the flat float32 parameter buffer in pinned host memory, as of everything enqueued so far"""
        snap = getattr(self, "_snap", None)
        if snap is None or snap["version"] != getattr(self, "_version", 0):
            ring, self._wring = getattr(self, "_wring", None), None       # (a private snapshot, not a ring publish)
            try:
                self.snapshot_weights_async()
            finally:
                self._wring = ring
            snap = self._snap
        snap["version"] = -1            # a pre-enqueued snapshot serves ONE publish; later calls copy again
        snap["events"][snap["slot"]].synchronize()
        return snap["host"][snap["slot"]].numpy()

    def publish_weights(self, ring, ctr_info=None, lag=0):
        """The learner's weight hand-over (xt/framework/learner.py:361-363) without an intermediate dict: the packed
        parameter block goes pinned block -> ring slot with one copy per variable, or -- when the ring is page-locked
        (``WeightsRing.pin``) -- by ONE D2H straight from HBM into the slot (no host copy at all).  Returns the
        publish's sequence number."""
        if getattr(ring, "pinned", False):
            attached = getattr(self, "_wring", None) is ring
            if getattr(ring, "async_commit", False):
                # the update enqueued the D2H into the ring slot (or it is enqueued now); the ring's committer thread makes it
                # visible when it lands -- this thread goes on (content = THIS update's weights, no lag)
                if not attached:
                    raise ValueError("publish_weights on a ring with an asynchronous committer needs attach_weights_ring(ring)")
                if getattr(self, "_wring_version", -1) != getattr(self, "_version", 0) or ctr_info:
                    ring.begin_flat_publish(self, ctr_info)
                    self._wring_version = getattr(self, "_version", 0)
                return ring._last_begun
            if lag > 0:
                # ``lag = 1`` (asynchronous algorithms, flagged deviation): hand out the weights whose copy was begun at the
                # PREVIOUS publish and never wait for the one just enqueued -- the next rollout message is ingested while
                # the GPU still runs this update.  The copy of the current update stays begun.  With
                # train_per_checkpoint = 1 every train begins a copy (eager_snapshot), so the lag is ONE TRAIN; with
                # train_per_checkpoint = k > 1 copies are only begun here, so the lag is one publish INTERVAL = k trains
                # (pong_impala_speedup.yaml: 3) -- bench.py labels it so.
                if not attached or ring.slots < 3:
                    raise ValueError("publish_weights(lag=1) needs attach_weights_ring(ring) and a ring of >= 3 slots")
                self._wring_lag = 1
                if not ring._pending or getattr(self, "_wring_version", -1) != getattr(self, "_version", 0):
                    ring.begin_flat_publish(self, ctr_info)
                    self._wring_version = getattr(self, "_version", 0)
                if len(ring._pending) > 1 or ring.latest() == 0:
                    return ring.commit_flat_publish()
                return ring.latest()
            self._wring_lag = 0
            if attached and ring._pending and getattr(self, "_wring_version", -1) == getattr(self, "_version", 0) and not ctr_info:
                while len(ring._pending) > 1:
                    ring.commit_flat_publish()
                return ring.commit_flat_publish()       # the update itself enqueued the copy (snapshot_weights_async)
            while ring._pending:
                ring.retarget_flat_publish()
            return ring.publish_flat_from_device(self, ctr_info)
        return ring.publish(self.get_weights(copy=False), ctr_info)

    def attach_weights_ring(self, ring):
        """From now on the weight snapshot that every update enqueues (``snapshot_weights_async``) lands directly in
        ``ring``'s next slot (``ring`` must be page-locked, ``WeightsRing.pin``): ``publish_weights(ring)`` then only
        waits for that copy and commits it.  ``None`` detaches."""
        if ring is not None and not getattr(ring, "pinned", False):
            raise ValueError("attach_weights_ring: the ring must be page-locked (WeightsRing.pin())")
        self._wring = ring

    def set_weights(self, weights):
        """Assign by name; unknown names are ignored, KeyError if nothing matches
        (TFVariables.set_weights, xt/model/tf_utils.py:104-128)."""
        hit = [k for k in weights.keys() if k in self.spec.names]
        if not hit:
            raise KeyError("NO node's weights could assign in self.graph {} vs {}".format(
                list(self.spec.names.keys()), list(weights.keys())))
        flat = self.params.detach().cpu().numpy().copy()
        for name in hit:
            off, shape = self.spec.names[name]
            val = np.asarray(weights[name], np.float32)
            if tuple(val.shape) != tuple(shape):
                raise KeyError("update {} encounter error: shape {} vs {}".format(name, val.shape, shape))
            self.spec.var_view(flat, name)[...] = val
        self.params.copy_(torch.from_numpy(flat))
        self.touch()

    # ------------------------------------------------------------------ optimizer state
    # The reference never checkpoints its AdamOptimizer slots (TFVariables only walks the trainable variables,
    # xt/model/tf_utils.py:60-97), so a restored run restarts Adam from zero.  For a true resume the slots are
    # exported under the names TF1 itself gives them ("<var>/Adam" = m, "<var>/Adam_1" = v, "beta1_power",
    # "beta2_power"), next to the weights: TFVariables.set_weights ignores names it does not know
    # (tf_utils.py:106-109), so the same .npz still loads in the reference.
    OPT_M, OPT_V, OPT_B1, OPT_B2, OPT_STEP = "/Adam", "/Adam_1", "beta1_power", "beta2_power", "adam_step"
    opt_kind = "adam"        # "rmsprop": the two slot buffers hold mg / ms; saved as "<var>/RMSProp_1" / "<var>/RMSProp"

    def _slot_suffixes(self):
        return ("/RMSProp_1", "/RMSProp") if self.opt_kind == "rmsprop" else (self.OPT_M, self.OPT_V)

    def get_optimizer_state(self):
        m = self.adam_m.detach().cpu().numpy()
        v = self.adam_v.detach().cpu().numpy()
        st = self.adam_state.detach().cpu().numpy()
        out = OrderedDict()
        for name in self.spec.names:
            sm, sv = self._slot_suffixes()
            out[name + sm] = self.spec.var_view(m, name).copy()
            out[name + sv] = self.spec.var_view(v, name).copy()
        out[self.OPT_B1] = np.float32(st[0])
        out[self.OPT_B2] = np.float32(st[1])
        out[self.OPT_STEP] = np.int64(round(float(st[5])))
        return out

    def set_optimizer_state(self, state):
        """Restore Adam slots saved by get_optimizer_state; returns False (state untouched) unless EVERY slot
        and both beta powers are present with the right shapes."""
        need = [n + sfx for n in self.spec.names for sfx in self._slot_suffixes()] + [self.OPT_B1, self.OPT_B2]
        if any(k not in state for k in need):
            return False
        m = np.zeros(self.spec.n_flat, np.float32)
        v = np.zeros(self.spec.n_flat, np.float32)
        for name, (off, shape) in self.spec.names.items():
            for sfx, dst in zip(self._slot_suffixes(), (m, v)):
                val = np.asarray(state[name + sfx], np.float32)
                if tuple(val.shape) != tuple(shape):
                    raise KeyError("optimizer slot {} shape {} vs {}".format(name + sfx, val.shape, shape))
                self.spec.var_view(dst, name)[...] = val
        st = self.adam_state.detach().cpu().numpy().copy()
        st[0], st[1] = np.float32(state[self.OPT_B1]), np.float32(state[self.OPT_B2])
        st[5] = np.float32(state[self.OPT_STEP]) if self.OPT_STEP in state else 0.0
        self.adam_m.copy_(torch.from_numpy(m))
        self.adam_v.copy_(torch.from_numpy(v))
        self.adam_state.copy_(torch.from_numpy(st))
        return True

    def check_device_errors(self):
        """Raise if a kernel flagged an error in the optimiser state block (state[6], include/xt_mi355x.h): today only
        the fused update tail (``xt_tuning.tail_fused``, off by default) whose grid barrier timed out and skipped an update."""
        flag = float(self.adam_state[6].item())
        if flag != 0.0:
            raise RuntimeError("xingtian_amd: device-side error word {} (1: the fused update tail's grid barrier timed "
                               "out, the update was skipped)".format(flag))

    def reset_optimizer(self):
        self.adam_m.zero_()
        self.adam_v.fill_(1.0) if self.opt_kind == "rmsprop" else self.adam_v.zero_()
        L.check(self.lib.xt_adam_state_init(L.ptr(self.adam_state), L.stream_ptr()), "xt_adam_state_init")

    # ------------------------------------------------------------------ compute
    def to_device_obs(self, obs):
        t = torch.as_tensor(np.ascontiguousarray(obs)) if not torch.is_tensor(obs) else obs
        want = torch.uint8 if self.spec.input_xform[0] else torch.float32
        t = t.to(device=self.device, dtype=want)
        lay0 = self.spec.layers[0]
        if t.dim() == 2 and lay0.H == lay0.W == 1 and t.shape[1] < lay0.C:      # zero-pad odd feature counts (netspec._mlp)
            t = torch.nn.functional.pad(t, (0, lay0.C - t.shape[1]))
        elif t.dim() == 4 and t.shape[3] < lay0.C:                                 # image channels -> multiple of 4
            t = self.pad_obs_channels(t.contiguous())
        return t.contiguous()

    def obs_fill_byte(self):
        """the uint8 value the input transform maps to 0 (what padded channel planes are filled with)"""
        is_u8, mean, _ = self.spec.input_xform
        if not is_u8 or mean == 0.0:
            return 0
        if float(mean) != int(mean) or not 0 <= int(mean) <= 255:
            raise ValueError("channel padding of uint8 observations needs an integral state_mean in [0, 255], got {}".format(mean))
        return int(mean)

    def pad_obs_channels(self, t, out=None):
        """[n, H, W, c] device tensor -> [n, H, W, pad4(c)] with neutral extra planes (C ABI xt_pad_channels)."""
        c_dst = self.spec.layers[0].C
        n, h, w, c = t.shape
        if out is None:
            out = torch.empty((n, h, w, c_dst), dtype=t.dtype, device=t.device)
        L.check(self.lib.xt_pad_channels(L.ptr(t), L.ptr(out), n * h * w, c, c_dst, t.element_size(), self.obs_fill_byte(),
                                         L.stream_ptr()), "xt_pad_channels")
        return out

    def forward(self, obs):
        """obs [B, ...] (host or device) -> (logits [B,A], value [B]) device tensors."""
        x = self.to_device_obs(obs)
        b = x.shape[0]
        a = self.spec.action_dim
        logits = torch.empty((b, a), dtype=torch.float32, device=self.device)
        value = torch.empty((b,), dtype=torch.float32, device=self.device)
        for s in range(0, b, self.max_batch):
            e = min(b, s + self.max_batch)
            L.check(self.lib.xt_net_forward(self.handle, L.ptr(x[s:e]), None, e - s, L.ptr(logits[s:e]),
                                            L.ptr(value[s:e]), L.stream_ptr()), "xt_net_forward")
        return logits, value

    ACT_MAX_ACTIONS = 64        # xt_net_act: one lane of the sample's wave per action

    def act(self, obs, seed, call, noise=None, want_noise=False):
        """``Model.predict`` on the device (C ABI ``xt_net_act``): obs [B, ...] -> dict of host arrays ``action`` (int32 [B] |
        float32 [B,A]), ``logp`` [B,1], ``value`` [B,1], ``logits`` [B,A] and -- ``want_noise`` -- ``noise`` [B,A], the Gumbel
        / standard-normal noise every action was drawn with.  ``noise`` [B,A] injects it instead of drawing from the
        counter-based generator keyed by (``seed``, ``call``, row, action).  All results land in ONE device block and reach
        the host by one copy into one pinned block and one synchronisation, however many ``max_batch`` chunks the batch
        takes.  The arrays are views of a private copy of that block."""
        x = self.to_device_obs(obs)
        b, a = int(x.shape[0]), self.spec.action_dim
        gauss = self._desc.action_type == L.ACTION_TYPE["DiagGaussian"]
        na = a if gauss else 1
        want_noise = bool(want_noise)
        blocks = getattr(self, "_act_blocks", None)
        if blocks is None:
            blocks = self._act_blocks = {}
        blk = blocks.get((b, a, want_noise))
        if blk is None:
            if len(blocks) >= 16:       # (a caller whose batch size keeps changing: do not hoard pinned memory)
                blocks.clear()
            # float32 words: action [b*na] | logp [b] | value [b] | logits [b*a] | noise [b*a]
            offs = np.cumsum([0, b * na, b, b, b * a, b * a if want_noise else 0])
            dev = torch.empty(int(offs[-1]), dtype=torch.float32, device=self.device)
            pin = torch.empty(int(offs[-1]), dtype=torch.float32, pin_memory=True)
            blk = blocks[(b, a, want_noise)] = dict(dev=dev, pin=pin, np=pin.numpy(), offs=[int(o) for o in offs],
                                                    base=dev.data_ptr(), cfg=L.ActCfg())
        noise_dev = None
        if noise is not None:
            noise_dev = torch.as_tensor(np.ascontiguousarray(noise, dtype=np.float32)).to(self.device).reshape(b, a)
        o_act, o_logp, o_val, o_lg, o_nz = blk["offs"][:5]
        cfg, base = blk["cfg"], blk["base"]
        cfg.seed, cfg.call = int(seed) & 0xFFFFFFFFFFFFFFFF, int(call) & 0xFFFFFFFFFFFFFFFF
        cfg.want_noise = 1 if want_noise else 0
        st = L.stream_ptr()
        for s in range(0, b, self.max_batch):
            e = min(b, s + self.max_batch)
            cfg.row0 = s
            L.check(self.lib.xt_net_act(
                self.handle, ctypes.byref(cfg), L.ptr(x[s:e]), None, e - s,
                L.ptr(noise_dev[s:e]) if noise_dev is not None else None, base + 4 * (o_act + s * na),
                base + 4 * (o_logp + s), base + 4 * (o_val + s), base + 4 * (o_lg + s * a),
                base + 4 * (o_nz + s * a) if want_noise else None, st), "xt_net_act")
        cur = L.current_stream(self.device)
        L.memcpy_async(blk["pin"].data_ptr(), base, blk["pin"].numel() * 4, L.D2H, cur)
        cur.synchronize()
        host = blk["np"].copy()
        action = host[o_act:o_logp].reshape(b, a) if gauss else host[o_act:o_logp].view(np.int32)
        out = dict(action=action, logp=host[o_logp:o_val].reshape(b, 1), value=host[o_val:o_lg].reshape(b, 1),
                   logits=host[o_lg:o_nz].reshape(b, a))
        if want_noise:
            out["noise"] = host[o_nz:].reshape(b, a)
        return out

    def set_dp(self, rank, world, loss_scale=1.0):
        """C ABI ``xt_net_set_dp``: switch the data-parallel tail on (``world`` >= 1: rows + loss shares of every rank travel
        behind the gradient in the same exchange, the optimiser adds the GLOBAL loss to ``loss_acc``) or off (``world`` = 0)"""
        L.check(self.lib.xt_net_set_dp(self.handle, int(rank), int(world), float(loss_scale)), "xt_net_set_dp")

    # ------------------------------------------------------------------ per-update training diagnostics (opt-in)
    train_stats_on = False

    def set_train_stats(self, on=True):
        """C ABI ``xt_net_set_train_stats``: switch the per-update PPO diagnostics on (the net then owns the 16 running sums
        and the [max_batch, 4] row scratch) or off.  Refused by the library while a data-parallel tail or a gradient
        exchange hook is attached."""
        if on:
            if getattr(self, "_tstats", None) is None:
                pin = torch.zeros((2, L.TRAIN_STATS_DOUBLES), dtype=torch.float64, pin_memory=True)
                self._tstats = dict(acc=torch.zeros(L.TRAIN_STATS_DOUBLES, dtype=torch.float64, device=self.device),
                                    rows=torch.zeros((self.max_batch, 4), dtype=torch.float32, device=self.device),
                                    pin=pin, np=pin.numpy(), slot=0, last=None)
            L.check(self.lib.xt_net_set_train_stats(self.handle, L.ptr(self._tstats["acc"]), L.ptr(self._tstats["rows"])),
                    "xt_net_set_train_stats")
        else:
            L.check(self.lib.xt_net_set_train_stats(self.handle, None, None), "xt_net_set_train_stats")
            if getattr(self, "_tstats", None) is not None:
                self._tstats["last"] = None
        self.train_stats_on = bool(on)

    def clear_train_stats(self):
        """zero the running sums (``xt_net_ppo_train`` does it itself; a caller of ``ppo_step`` does it here)"""
        self._tstats["acc"].zero_()

    def enqueue_train_stats(self):
        """One 128-byte D2H of the running sums into the next of two alternating pinned blocks, in stream order behind
        everything enqueued so far and with no synchronisation of its own: ``read_loss`` records and awaits its event
        behind this copy, so the block is complete once the loss is."""
        ts = self._tstats
        i = ts["slot"]
        L.memcpy_async(ts["pin"][i].data_ptr(), ts["acc"].data_ptr(), 8 * L.TRAIN_STATS_DOUBLES, L.D2H,
                       L.current_stream(self.device))
        ts["slot"], ts["last"] = i ^ 1, i

    def train_stats_sums(self):
        """float64 [16]: the sums the last ``enqueue_train_stats`` copied (None before the first); valid once a
        ``read_loss`` behind it has returned"""
        ts = getattr(self, "_tstats", None)
        if ts is None or ts["last"] is None:
            return None
        return ts["np"][ts["last"]].copy()

    def last_head_path(self):
        """the head / loss kernel the most recent PPO or IMPALA step launched (C ABI ``xt_net_last_head_path``; diagnostic)"""
        return int(self.lib.xt_net_last_head_path(self.handle))

    def last_step_report(self):
        """what the most recent step decided from the net's shapes (C ABI ``xt_net_last_step_report``, ``lib.step_report``;
        host words only, diagnostic)"""
        return L.step_report(self.handle)

    def graph_cache_info(self):
        """captures / launches / evictions / live slots of the net's update-graph cache (C ABI ``xt_net_graph_cache_info``,
        ``lib.graph_cache_info``; host words only, diagnostic)"""
        return L.graph_cache_info(self.handle)

    gauss_fused_on = False

    def set_gauss_fused(self, on=True):
        """C ABI ``xt_net_set_gauss_fused``: a DiagGaussian PPO step inside the fused head kernel's envelope (A <= 8,
        features <= 512) runs ``ppo_gauss_heads_fused_kernel`` instead of heads forward + loss + heads d(features).  Off by
        default; refused by the library on a categorical net."""
        L.check(self.lib.xt_net_set_gauss_fused(self.handle, 1 if on else 0), "xt_net_set_gauss_fused")
        self.gauss_fused_on = bool(on)

    fwd_fuse12_flat_on = True

    def set_fwd_fuse12_flat(self, on=True):
        """C ABI ``xt_net_set_fwd_fuse12_flat``: PpoCnn's conv1 -> conv2 forward as ONE launch
        (``conv12_u8_valid_fwd_flat_kernel``) where the batch is inside the kernel's envelope, bit for bit the two
        launches' results.  On by default; ``False`` keeps the two launches everywhere."""
        L.check(self.lib.xt_net_set_fwd_fuse12_flat(self.handle, 1 if on else 0), "xt_net_set_fwd_fuse12_flat")
        self.fwd_fuse12_flat_on = bool(on)

    fwd_fuse123_flat_on = True

    def set_fwd_fuse123_flat(self, on=True):
        """C ABI ``xt_net_set_fwd_fuse123_flat``: PpoCnn's conv1 -> conv2 -> conv3 forward as ONE launch
        (``conv123_u8_valid_fwd_flat_kernel``) where the batch is inside that kernel's envelope (201 .. 320 frames of
        84x84), bit for bit the separate launches' results.  On by default; needs ``set_fwd_fuse12_flat`` on."""
        L.check(self.lib.xt_net_set_fwd_fuse123_flat(self.handle, 1 if on else 0), "xt_net_set_fwd_fuse123_flat")
        self.fwd_fuse123_flat_on = bool(on)

    # ------------------------------------------------------------------ per-train IMPALA v-trace diagnostics (opt-in)
    impala_stats_on = False

    def set_impala_stats(self, on=True):
        """C ABI ``xt_net_set_impala_stats``: switch the per-train v-trace diagnostics on (the net then owns the 16 running
        sums and one row of scratch per trajectory a chunk can hold) or off.  Refused by the library while a data-parallel
        tail, a gradient exchange hook or a direct comm is attached."""
        if on:
            if getattr(self, "_istats", None) is None:
                rows = max(int(self.max_batch) // 2, 1)         # (a trajectory has at least two frames)
                pin = torch.zeros(L.IMPALA_STATS_DOUBLES, dtype=torch.float64, pin_memory=True)
                self._istats = dict(acc=torch.zeros(L.IMPALA_STATS_DOUBLES, dtype=torch.float64, device=self.device),
                                    traj=torch.zeros((rows, L.IMPALA_TRAJ_STATS_FLOATS), dtype=torch.float32,
                                                     device=self.device), rows=rows, pin=pin, np=pin.numpy())
            ts = self._istats
            L.check(self.lib.xt_net_set_impala_stats(self.handle, L.ptr(ts["acc"]), L.ptr(ts["traj"]), ts["rows"]),
                    "xt_net_set_impala_stats")
        else:
            L.check(self.lib.xt_net_set_impala_stats(self.handle, None, None, 0), "xt_net_set_impala_stats")
        self.impala_stats_on = bool(on)

    def clear_impala_stats(self):
        """zero the running sums (``xt_net_impala_train`` does it itself; a caller of ``impala_step`` does it here)"""
        self._istats["acc"].zero_()

    def fetch_impala_stats(self):
        """float64 [16]: the running sums as the work enqueued so far leaves them -- ONE 128-byte D2H into a pinned block
        and one wait for the stream, both issued by this call (nothing rides behind a train when nobody asks)"""
        ts = self._istats
        cur = L.current_stream(self.device)
        L.memcpy_async(ts["pin"].data_ptr(), ts["acc"].data_ptr(), 8 * L.IMPALA_STATS_DOUBLES, L.D2H, cur)
        torch.cuda.current_stream(self.device).synchronize()
        return ts["np"].copy()

    def read_loss(self, acc=None, wait=True):
        """[sum of step losses, number of steps, data-parallel error bits, -] of the train(s) enqueued so far: ONE 16-byte D2H
        into a pinned block + an event wait instead of a pageable ``.cpu()`` (a staging copy, an allocation and a device-wide
        synchronisation: ~30 us of a 128-frame IMPALA train).  Two blocks alternate; ``wait=False`` returns the block of the
        PREVIOUS call instead (ASYNC_LOSS: its copy landed long ago; the very first call still waits for its own).  Raises if
        the train left error bits (the update was skipped on this rank: include/xt_mi355x.h ``xt_net_set_direct``)."""
        acc = self.loss_acc if acc is None else acc
        rb = getattr(self, "_loss_rb", None)
        if rb is None:
            pin = torch.zeros((2, 4), dtype=torch.float32, pin_memory=True)
            rb = self._loss_rb = dict(pin=pin, np=pin.numpy(), ev=[torch.cuda.Event(), torch.cuda.Event()], slot=0, n=0)
        i = rb["slot"]
        cur = L.current_stream(self.device)
        L.memcpy_async(rb["pin"][i].data_ptr(), acc.data_ptr(), 16, L.D2H, cur)
        rb["ev"][i].record(cur)
        rb["slot"] = i ^ 1
        j = i if (wait or rb["n"] == 0) else i ^ 1
        rb["n"] += 1
        gate = getattr(self, "idle_gate", None)        # (transport.Prefetcher: its staging thread works while we wait)
        if gate is not None:
            gate.set()
            rb["ev"][j].synchronize()
            gate.clear()
        else:
            rb["ev"][j].synchronize()
        a = rb["np"][j]
        if a[2] != 0.0:
            raise RuntimeError("xingtian_amd: the data-parallel update failed on this rank -- {} (error bits {}); the "
                               "optimiser skipped the update, parameters are those of the last good step".format(
                                   L.dp_error_text(a[2]), int(a[2])))
        return a

    def make_ppo_cfg(self, cfg, grad_scale=1.0, global_batch=0, shard_rank=0, shard_world=0):
        c = L.PpoCfg()
        c.lr, c.beta1, c.beta2, c.eps = cfg["LR"], 0.9, 0.999, 1e-8
        c.clip_ratio, c.ent_coef, c.vf_clip = cfg["LOSS_CLIPPING"], cfg["ENTROPY_LOSS"], cfg["VF_CLIP"]
        c.critic_coef, c.max_grad_norm = cfg["CRITIC_LOSS_COEF"], cfg["MAX_GRAD_NORM"]
        c.batch_size, c.num_sgd_iter = int(cfg["BATCH_SIZE"]), int(cfg["NUM_SGD_ITER"])
        c.grad_scale, c.global_batch = grad_scale, int(global_batch)
        # strict data parallelism inside xt_net_ppo_train: this rank's shard of every global minibatch (ABI >= 9)
        c.shard_rank, c.shard_world = int(shard_rank), int(shard_world)
        return c

    def ppo_step(self, c, obs, idx, action, old_logp, adv, old_v, target_v, apply=True):
        """One SGD step on rows idx (int32 device tensor or None) of device-resident data."""
        b = int(idx.numel()) if idx is not None else int(obs.shape[0])
        self.touch()
        L.check(self.lib.xt_net_ppo_step(self.handle, ctypes.byref(c), L.ptr(obs), L.ptr(idx), b, L.ptr(action),
                                         L.ptr(old_logp), L.ptr(adv), L.ptr(old_v), L.ptr(target_v),
                                         1 if apply else 0, L.ptr(self.loss_out), None, L.stream_ptr()),
                "xt_net_ppo_step")
        return self.loss_out

    def ppo_train(self, c, obs, perm, action, old_logp, adv, old_v, target_v, use_graph=False):
        n = int(obs.shape[0])
        self.touch()
        L.check(self.lib.xt_net_ppo_train(self.handle, ctypes.byref(c), L.ptr(obs), n, L.ptr(perm), L.ptr(action),
                                          L.ptr(old_logp), L.ptr(adv), L.ptr(old_v), L.ptr(target_v),
                                          L.ptr(self.loss_acc), 1 if use_graph else 0, L.stream_ptr()),
                "xt_net_ppo_train")
        return self.loss_acc

    def make_impala_cfg(self, lr, grad_norm_clip, sample_batch_step, gamma=0.99, grad_scale=1.0, opt_type="adam",
                        shard_rank=0, shard_world=0):
        c = L.ImpalaCfg()
        c.shard_rank, c.shard_world = int(shard_rank), int(shard_world)
        c.lr, c.beta1, c.beta2, c.eps = lr, 0.9, 0.999, 1e-8
        c.grad_norm_clip, c.gamma, c.sample_batch_step, c.grad_scale = grad_norm_clip, gamma, int(sample_batch_step), grad_scale
        c.opt_type = L.OPT_TYPE[opt_type]
        c.rms_decay, c.rms_eps = 0.99, 0.1          # RMSPropOptimizer(LR, decay=0.99, epsilon=0.1, centered=True)
        if opt_type != self.opt_kind:
            raise ValueError("call set_optimizer({!r}) before building its config".format(opt_type))
        return c

    def set_optimizer(self, kind):
        """'adam' (default) or 'rmsprop': the latter reuses the two slot buffers as mean gradient / mean square and
        initialises them as TF does (rms = ones, mg = zeros)."""
        if kind not in L.OPT_TYPE:
            raise KeyError("invalid opt_type: {}".format(kind))
        self.opt_kind = kind
        self.reset_optimizer()

    def impala_step(self, c, obs, bp_logits, action, done, reward, apply=True, loss_acc=None):
        n = int(obs.shape[0])
        self.touch()
        L.check(self.lib.xt_net_impala_step(self.handle, ctypes.byref(c), L.ptr(obs), n, L.ptr(bp_logits),
                                            L.ptr(action), L.ptr(done), L.ptr(reward), 1 if apply else 0,
                                            L.ptr(self.loss_out), L.ptr(loss_acc), L.stream_ptr()),
                "xt_net_impala_step")
        return self.loss_out

    def impala_train(self, c, obs, batch_size, bp_logits, action, done, reward, lr_steps=None, use_graph=False):
        """IMPALAOpt.train in one call (C ABI xt_net_impala_train): sequential BATCH_SIZE chunks of the resident
        rollout; ``lr_steps`` (float32 device tensor, one step size per chunk) or None.  Returns the device tensor
        [sum of chunk losses, number of chunks]."""
        n = int(obs.shape[0])
        self.touch()
        L.check(self.lib.xt_net_impala_train(self.handle, ctypes.byref(c), L.ptr(obs), n, int(batch_size),
                                             L.ptr(bp_logits), L.ptr(action), L.ptr(done), L.ptr(reward),
                                             L.ptr(lr_steps), L.ptr(self.loss_acc), 1 if use_graph else 0,
                                             L.stream_ptr()), "xt_net_impala_train")
        return self.loss_acc

    def impala_train_io(self, c, obs, batch_size, bp_logits, action, done, reward, lr_steps=None, use_graph=False,
                        wait_event=None, consumed_event=None, publish=None, wait_loss=True, tail_in_graph=True, defer=False,
                        wait_dma_ticket=0):
        """``impala_train`` + the runtime calls of the learner loop around it in ONE C call (``xt_net_impala_train_io``): the
        compute stream waits for ``wait_event`` (the rollout's copies), ``consumed_event`` is recorded behind the train,
        ``loss_acc`` is copied into the next pinned read-back block and -- ``wait_loss`` -- awaited with the GIL released,
        ``publish`` = (host address of a pinned weights-ring slot, raw event handle) receives the new parameters by a D2H in
        stream order behind the loss copy (``WeightsRing.publish_reserve``).  ``tail_in_graph`` (with ``wait_loss``): both
        copies are the train's own last kernels, inside its replayed hipGraph, and the loss is awaited by polling a
        page-locked word (``xt_train_io.tail_in_graph``); ``defer`` (with both): return right behind the launch -- the caller
        does its loss-independent book-keeping under the device's train and fetches the loss with ``impala_wait_loss()``.
        Returns the pinned [sum, count, error bits, -] block of THIS train (``wait_loss``) or of the previous one (None when
        deferred); raises on error bits."""
        n = int(obs.shape[0])
        self._version = getattr(self, "_version", 0) + 1          # touch()
        rb = getattr(self, "_loss_rb", None)
        if rb is None:
            pin = torch.zeros((2, 4), dtype=torch.float32, pin_memory=True)
            rb = self._loss_rb = dict(pin=pin, np=pin.numpy(), ev=[torch.cuda.Event(), torch.cuda.Event()], slot=0, n=0)
        if "raw" not in rb:
            cur = L.current_stream(self.device)
            for ev in rb["ev"]:
                ev.record(cur)                 # (a torch event gets its handle at its first record)
            rb["raw"] = [ev.cuda_event for ev in rb["ev"]]
            rb["ptr"] = [rb["pin"][k].data_ptr() for k in range(2)]
            rb["io"] = L.TrainIO()             # one descriptor, rewritten per train
            rb["io_ref"] = ctypes.byref(rb["io"])
            rb["fn"] = self.lib.xt_net_impala_train_io
            rb["dev"] = self.device.index if self.device.index is not None else torch.cuda.current_device()
            rb["acc"] = self.loss_acc.data_ptr()
        i = rb["slot"]
        io = rb["io"]
        io.wait_event = wait_event.cuda_event if wait_event is not None else None
        io.wait_dma_ticket = int(wait_dma_ticket)      # (xt_dma_h2d_async copies of the rollout: awaited before the launch)
        io.consumed_event = consumed_event.cuda_event if consumed_event is not None else None
        if publish is not None:
            io.publish_dst, io.publish_event = publish[0], publish[1]
        else:
            io.publish_dst, io.publish_event = None, None
        sync = bool(wait_loss or rb["n"] == 0)
        tail = bool(tail_in_graph and sync)
        deferred = bool(defer and tail)
        io.loss_host, io.loss_event, io.wait_loss = rb["ptr"][i], rb["raw"][i], (2 if deferred else 1) if sync else 0
        io.tail_in_graph = (2 if int(tail_in_graph) == 2 else 1) if tail else 0      # (2: snapshot + side-stream D2H)
        ptr = L.ptr
        # the staging thread may work while this thread is inside C with the GIL released -- in the deferred form only from
        # impala_wait_loss() on: the launch is ~15 us and the book-keeping behind it needs the GIL to itself (two Python
        # threads hand it back and forth at every runtime call: measured, the 16 us C call took 56-67 us with the gate open)
        gate = getattr(self, "idle_gate", None)
        if deferred and not getattr(self, "gate_at_launch", True):
            gate = None
        if gate is not None:
            gate.set()
        try:
            rc = rb["fn"](self.handle, ctypes.byref(c), ptr(obs), n, int(batch_size), ptr(bp_logits), ptr(action), ptr(done),
                          ptr(reward), ptr(lr_steps), rb["acc"], 1 if use_graph else 0, rb["io_ref"],
                          torch._C._cuda_getCurrentRawStream(rb["dev"]))
            if rc:
                L.check(rc, "xt_net_impala_train_io")
        finally:
            if gate is not None and not deferred:
                gate.clear()
        rb["slot"] = i ^ 1
        rb["n"] += 1
        if deferred:
            rb["deferred"] = i
            return None
        j = i if sync else i ^ 1
        if j != i:
            rb["ev"][j].synchronize()
        return self._loss_block(rb["np"][j])

    def io_publish_done(self):
        """completion handle (``synchronize()`` / ``query()``, the two calls a ``transport.WeightsRing`` makes on a publish's
        event) of the parameter copy of the most recent ``tail_in_graph`` train: the copy kernel's last workgroup writes the
        train's sequence number into the mailbox (C ABI ``xt_net_io_seq`` / ``xt_net_io_publish_wait``) -- no event record
        behind the replayed graph"""
        return _MailboxDone(self, int(self.lib.xt_net_io_seq(self.handle)))

    def impala_wait_loss(self):
        """second half of ``impala_train_io(..., defer=True)``: wait for that train's loss (C ABI ``xt_net_io_wait``, GIL
        released) -> its pinned [sum, count, error bits, -] block"""
        rb = self._loss_rb
        i = rb.pop("deferred")
        # an INLINE prefetcher (transport.Prefetcher(inline=True)): this thread stages the next rollout message(s) itself while
        # the device trains -- one interpreter thread, nobody to fight for the lock -- and looks at the mailbox in between
        hook = getattr(self, "idle_hook", None)
        if hook is not None:
            ready = self.lib.xt_net_io_loss_ready
            while not ready(self.handle):
                if not hook():
                    break               # (nothing to stage: wait in C below)
        gate = getattr(self, "idle_gate", None)
        if gate is not None:
            gate.set()
        try:
            rc = self.lib.xt_net_io_wait(self.handle, rb["ptr"][i], torch._C._cuda_getCurrentRawStream(rb["dev"]))
            if rc:
                L.check(rc, "xt_net_io_wait")
        finally:
            if gate is not None:
                gate.clear()
        return self._loss_block(rb["np"][i])

    @staticmethod
    def _loss_block(a):
        if a[2] != 0.0:
            raise RuntimeError("xingtian_amd: the data-parallel update failed on this rank -- {} (error bits {}); the "
                               "optimiser skipped the update, parameters are those of the last good step".format(
                                   L.dp_error_text(a[2]), int(a[2])))
        return a

    def io_times(self, reset=True):
        """host time per call (us) of the phases of ``impala_train_io`` -- before the launch, the launch, the runtime calls
        behind it, the wait for the loss (C ABI ``xt_net_io_times``; diagnostic)"""
        us, calls = (ctypes.c_double * 4)(), ctypes.c_int64()
        L.check(self.lib.xt_net_io_times(self.handle, us, ctypes.byref(calls), 1 if reset else 0), "xt_net_io_times")
        n = max(int(calls.value), 1)
        return dict(calls=int(calls.value), pre_us=us[0] / n, launch_us=us[1] / n, post_us=us[2] / n, wait_us=us[3] / n)

    def keras_impala_step(self, obs, idx, adv, onehot, target_v, ent_coef, loss_acc=None):
        """One ``model.fit`` minibatch of the non-opt IMPALA models (C ABI xt_net_keras_impala_step): forward, Keras
        impala_loss + 0.5 mse, backward; the gradient stays in ``self.grads`` for ``adam_keras``.  Returns the device
        tensor [loss, policy loss, mse]."""
        b = int(idx.numel()) if idx is not None else int(obs.shape[0])
        L.check(self.lib.xt_net_keras_impala_step(self.handle, L.ptr(obs), L.ptr(idx), b, L.ptr(adv), L.ptr(onehot),
                                                  L.ptr(target_v), float(ent_coef), L.ptr(self.loss_out),
                                                  L.ptr(loss_acc) if loss_acc is not None else None, L.stream_ptr()),
                "xt_net_keras_impala_step")
        return self.loss_out

    def adam_keras(self, lr, iterations, clipnorm=0.0, decay=0.0, beta1=0.9, beta2=0.999, eps=1e-7):
        """tf.keras Adam on the flat buffers: per-TENSOR clip_by_norm (kernel and bias are separate tensors), time-decayed
        learning rate; ``iterations`` = number of updates applied so far."""
        offs, sizes, n = self._keras_segments()
        lr_t = keras_lr_t(lr, iterations, decay, beta1, beta2)
        self.touch()
        L.check(self.lib.xt_adam_keras(L.ptr(self.params), L.ptr(self.grads), L.ptr(self.adam_m), L.ptr(self.adam_v), n,
                                       offs.data_ptr(), sizes.data_ptr(), float(clipnorm), float(lr_t), beta1, beta2,
                                       eps, L.ptr(self._keras_scratch), L.stream_ptr()), "xt_adam_keras")

    def _keras_segments(self):
        """(offsets, sizes, count) of the parameter TENSORS in the flat buffer (host int64 tensors) for ``xt_adam_keras``'s
        per-tensor clip; allocates its device scratch on first use."""
        if not hasattr(self, "_keras_segs"):
            offs, sizes = [], []
            for name in self.spec.names:      # (a channel-padded kernel: its storage block; the padding is zero)
                off, size = self.spec.var_extent(name)
                offs.append(int(off))
                sizes.append(int(size))
            dev = self.device
            self._keras_segs = (torch.tensor(offs, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64), len(offs))
            self._keras_scratch = torch.zeros((16 * len(offs),), dtype=torch.float32, device=dev)
        return self._keras_segs

    def keras_impala_train(self, obs, n_frag, t, onehot, behaviour, reward, done, idx, table, gamma, ent_coef,
                           clipnorm=0.0, beta1=0.9, beta2=0.999, eps=1e-7):
        """One whole train of the non-opt IMPALA in one C call that never synchronises (C ABI
        ``xt_net_keras_impala_train``): forward over the ``n_frag * (t + 1)`` resident observation rows, the float64
        v-trace kernel, then every minibatch of ``table`` (``keras_fit_table``) with its own Adam step.  All per-transition
        device arrays are in observation-ROW layout (row ``f * (t + 1) + s``, slot ``s = t`` unused); ``idx`` (int32,
        device) holds observation rows.  -> dict of the device buffers it filled: ``logits`` / ``value`` / ``pg_adv`` /
        ``target`` [rows] and ``acc`` [chunks, 2] (epoch loss of chunk c = acc[c, 0] / acc[c, 1])."""
        rows, a = int(n_frag) * (int(t) + 1), self.spec.action_dim
        want = {"obs": (obs, rows, None), "onehot": (onehot, rows * a, torch.float32),
                "behaviour": (behaviour, rows * a, torch.float32), "reward": (reward, rows, torch.float64),
                "done": (done, rows, torch.uint8), "idx": (idx, None, torch.int32)}
        for name, (x, numel, dtype) in want.items():
            ok = x.is_cuda and x.is_contiguous() and (dtype is None or x.dtype == dtype)
            ok = ok and (numel is None or (x.shape[0] == rows if name == "obs" else x.numel() == numel))
            if not ok:
                raise ValueError("keras_impala_train: {} must be a contiguous device tensor in row layout "
                                 "({} rows)".format(name, rows))
        if not table or any(off < 0 or off + n > idx.numel() for off, n, _, _ in table):
            raise ValueError("keras_impala_train: the minibatch table does not fit idx ({} entries)".format(idx.numel()))
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=self.device)
        n_chunks = max(e[2] for e in table) + 1
        out = dict(logits=new(rows, a), value=new(rows), pg_adv=new(rows), target=new(rows), acc=new(n_chunks, 2))
        offs, sizes, n_seg = self._keras_segments()
        cfg = L.KerasTrainCfg(float(ent_coef), float(clipnorm), beta1, beta2, eps, float(gamma), n_seg, offs.data_ptr(),
                              sizes.data_ptr(), self._keras_scratch.data_ptr())
        tab = (L.KerasFitEntry * len(table))(*table)
        self.touch()
        L.check(self.lib.xt_net_keras_impala_train(
            self.handle, ctypes.byref(cfg), L.ptr(obs), obs[0].numel() * obs.element_size(), int(n_frag), int(t),
            L.ptr(onehot), L.ptr(behaviour), L.ptr(reward), L.ptr(done), L.ptr(out["logits"]), L.ptr(out["value"]),
            L.ptr(out["pg_adv"]), L.ptr(out["target"]), L.ptr(idx), int(idx.numel()), tab, len(table), n_chunks,
            L.ptr(out["acc"]), L.stream_ptr()), "xt_net_keras_impala_train")
        return out

    def dqn_step(self, target, cur_ring, next_ring, slots, action, reward, done, gamma, dueling, double_dqn,
                 follow=None, n=1, per=None, dist=False, loss_acc=None, quant=False):
        """One ``DQN.train`` up to the gradient (never synchronises): the minibatch ``slots`` (int32, device) is gathered
        out of the device rings ``cur_ring`` / ``next_ring`` [capacity, ...] (rows as ``to_device_obs`` lays them out),
        ``target`` (a second ``HipActorCritic`` of the same spec) evaluates the next states, this net the states; the TD /
        MSE head reads ``action`` int32 / ``reward`` float64 / ``done`` uint8 [capacity] through the same slots.  The
        gradient stays in ``self.grads`` for ``adam_keras``.  Returns the device tensor [loss, mean |TD error|, mean
        bootstrap Q].

        ``per`` (a dict: size, u, sum_tree, min_tree, max_prio, alpha, beta, eps, optionally terms_out): prioritised
        replay; ``slots`` is ignored, the minibatch is drawn on the device from the sum tree with the float64 uniform
        draws ``u`` [B] over the ``size`` stored transitions, the head is weighted with the importance weights, and the
        sampled leaves of ``sum_tree`` / ``min_tree`` (float64 [2 * cap2]) and ``max_prio`` (float64 [1]) take the new TD
        errors.  The sampled slots and weights stay in ``self.per_slots`` / ``self.per_weights`` [max_batch];
        ``terms_out`` (float32 [2 * B]) receives (TD error, bootstrap Q) per sample.

        ``follow`` (int32 [capacity]: how many rows follow each slot in its message) with ``n``: n-step targets; the
        next-state gather walks every start slot over the up to ``n - 1`` rows behind it, both next-state forwards run
        on the rows it arrives at, and the head reads the discounted reward sum, ``gamma ** m`` and the last row's
        ``done``.  New priorities go to the start slots.  The labels of the walk stay in ``self.nstep_boot`` /
        ``nstep_action`` / ``nstep_reward`` / ``nstep_disc`` / ``nstep_done`` [max_batch].

        ``dist``: the categorical projection and cross-entropy head ``xt_dqn_loss_dist`` of a distributional pair (both
        nets carry the mark of ``set_dist``; no ``dueling`` -- a dueling distributional pair carries the mark of ``set_duel``
        on both nets and the entry reads it); the new priority of a start slot is its loss + eps and the
        tensor returned is [loss, mean per-sample loss, mean bootstrap Q].

        ``quant``: the quantile-Huber head ``xt_dqn_loss_quant`` of a quantile pair (both nets carry the mark of
        ``set_quant``; no dueling), with the priorities and the returned tensor of ``dist``.

        The C entry follows from the arguments alone, the first row that applies:

            quant                 xt_net_dqn_step_quant
            dist                  xt_net_dqn_step_dist
            follow is not None    xt_net_dqn_step_n
            per is not None       xt_net_dqn_step_per
            otherwise             xt_net_dqn_step
        """
        who = "dqn_step" + ("_quant" if quant else "_dist" if dist else "_n" if follow is not None else "_per" if per is not None else "")
        cap, row_bytes, cfg = self._dqn_cfg(who, cur_ring, next_ring, {"slots": slots} if per is None else {"u": per["u"]},
                                            action, reward, done, gamma, dueling, double_dqn)
        if per is None:
            b, size, p_ref, slots_ptr = int(slots.numel()), 0, None, L.ptr(slots)
        else:
            b, p = self._per_cfg(who, **{k: v for k, v in per.items() if k != "size"})
            size, p_ref, slots_ptr = int(per["size"]), ctypes.byref(p), None
        ns_ref = None
        if follow is not None:
            ns = self._nstep_cfg(who, follow, n, cap)
            ns_ref = ctypes.byref(ns)
        front, back = self._DQN_ENTRY_ARGS[who](ns_ref, p_ref, size, slots_ptr)
        entry = "xt_net_" + who
        L.check(getattr(self.lib, entry)(
            self.handle, target.handle, ctypes.byref(cfg), *front, L.ptr(cur_ring), L.ptr(next_ring), row_bytes, cap, *back, b,
            L.ptr(action), L.ptr(reward), L.ptr(done), L.ptr(self.loss_out),
            L.ptr(loss_acc) if loss_acc is not None else None, L.stream_ptr()), entry)
        return self.loss_out

    # what each C entry takes besides the arguments all five share: (after the cfg, after the rings' capacity)
    _DQN_ENTRY_ARGS = {
        "dqn_step": lambda ns, p, size, slots: ((), (slots,)),
        "dqn_step_per": lambda ns, p, size, slots: ((p,), (size,)),
        "dqn_step_n": lambda ns, p, size, slots: ((ns, p), (size, slots)),
        "dqn_step_dist": lambda ns, p, size, slots: ((ns, p), (size, slots)),
        "dqn_step_quant": lambda ns, p, size, slots: ((ns, p), (size, slots)),
    }

    # The three names from before ``dqn_step`` took keywords, each forwarding with its old argument order.  Nothing in the
    # package calls them; they stay for one step so that callers and tests written against the previous surface keep
    # running on this one, and go (with tests/test_gpu_dqn.py::test_net_dqn_step_earlier_names_forward_to_it) in the next.
    def dqn_step_per(self, target, cur_ring, next_ring, size, u, action, reward, done, gamma, dueling, double_dqn,
                     sum_tree, min_tree, max_prio, alpha, beta, eps, terms_out=None, loss_acc=None):
        per = dict(size=size, u=u, sum_tree=sum_tree, min_tree=min_tree, max_prio=max_prio, alpha=alpha, beta=beta, eps=eps,
                   terms_out=terms_out)
        return self.dqn_step(target, cur_ring, next_ring, None, action, reward, done, gamma, dueling, double_dqn, per=per,
                             loss_acc=loss_acc)

    def dqn_step_n(self, target, cur_ring, next_ring, slots, action, reward, done, follow, n, gamma, dueling, double_dqn,
                   per=None, loss_acc=None):
        return self.dqn_step(target, cur_ring, next_ring, slots, action, reward, done, gamma, dueling, double_dqn, follow, n,
                             per, loss_acc=loss_acc)

    def dqn_step_dist(self, target, cur_ring, next_ring, slots, action, reward, done, gamma, double_dqn, follow=None, n=1,
                      per=None, loss_acc=None):
        return self.dqn_step(target, cur_ring, next_ring, slots, action, reward, done, gamma, False, double_dqn, follow, n,
                             per, True, loss_acc)

    def _dqn_cfg(self, who, cur_ring, next_ring, batch, action, reward, done, gamma, dueling, double_dqn):
        """-> (capacity, row_bytes, ``DqnCfg``) after the tensor checks of ``dqn_step``; ``batch``:
        the per-sample device tensors by name (int32 slots / float64 draws)"""
        cap = int(cur_ring.shape[0])
        row_bytes = cur_ring[0].numel() * cur_ring.element_size()
        want = {"cur_ring": (cur_ring, None), "next_ring": (next_ring, cur_ring.dtype),
                "action": (action, torch.int32), "reward": (reward, torch.float64), "done": (done, torch.uint8)}
        want.update({k: (x, torch.int32 if k == "slots" else torch.float64) for k, x in batch.items()})
        for name, (x, dtype) in want.items():
            ok = x.is_cuda and x.is_contiguous() and (dtype is None or x.dtype == dtype)
            if not (ok and (name in batch or x.shape[0] == cap)):
                raise ValueError("{}: {} must be a contiguous device tensor ({} rows)".format(who, name, cap))
        if next_ring.shape != cur_ring.shape:
            raise ValueError("{}: the two state rings differ in shape".format(who))
        a = self.spec.action_dim                        # (the head's width: actions * atoms of a distributional spec)
        if not hasattr(self, "_dqn_scratch"):
            mb = self.max_batch
            self._dqn_scratch = (torch.empty((mb, row_bytes), dtype=torch.uint8, device=self.device),
                                 torch.empty((mb, row_bytes), dtype=torch.uint8, device=self.device),
                                 torch.empty((2 * mb * (a + 1),), dtype=torch.float32, device=self.device))
        cur_rows, next_rows, q = self._dqn_scratch
        return cap, row_bytes, L.DqnCfg(float(gamma), int(bool(dueling)), int(bool(double_dqn)), cur_rows.data_ptr(),
                                        next_rows.data_ptr(), q.data_ptr())

    def _per_cfg(self, who, u, sum_tree, min_tree, max_prio, alpha, beta, eps, terms_out=None):
        """-> (B, ``PerCfg``) after the tensor checks of the prioritised steps; allocates ``per_slots`` / ``per_weights``"""
        cap2 = int(sum_tree.numel()) // 2
        for name, x, n in (("sum_tree", sum_tree, 2 * cap2), ("min_tree", min_tree, 2 * cap2), ("max_prio", max_prio, 1)):
            if not (x.is_cuda and x.is_contiguous() and x.dtype == torch.float64 and x.numel() == n):
                raise ValueError("{}: {} must be a contiguous float64 device tensor of {} elements".format(who, name, n))
        b = int(u.numel())
        if terms_out is not None and not (terms_out.is_cuda and terms_out.is_contiguous() and
                                          terms_out.dtype == torch.float32 and terms_out.numel() >= 2 * b):
            raise ValueError("{}: terms_out must be a contiguous float32 device tensor of 2 * B elements".format(who))
        if not hasattr(self, "per_slots"):
            self.per_slots = torch.zeros(self.max_batch, dtype=torch.int32, device=self.device)
            self.per_weights = torch.zeros(self.max_batch, dtype=torch.float64, device=self.device)
        return b, L.PerCfg(sum_tree.data_ptr(), min_tree.data_ptr(), cap2, max_prio.data_ptr(), u.data_ptr(),
                           self.per_slots.data_ptr(), self.per_weights.data_ptr(),
                           terms_out.data_ptr() if terms_out is not None else None, float(alpha), float(beta), float(eps))

    def set_dist(self, atoms, v_min, v_max):
        """Mark the net as carrying a distributional Q head of ``atoms`` atoms on [v_min, v_max] (C ABI
        ``xt_net_set_dist``; ``spec.action_dim`` is actions * atoms); ``atoms`` 1 clears the mark."""
        L.check(self.lib.xt_net_set_dist(self.handle, int(atoms), float(v_min), float(v_max)), "xt_net_set_dist")
        self.dist = (int(atoms), float(v_min), float(v_max)) if int(atoms) > 1 else None
        if self.dist is None:
            self.duel = False                           # (clearing the mark clears the dueling one)

    def set_quant(self, quantiles, kappa):
        """Mark the net as carrying a quantile (QR-DQN) Q head of ``quantiles`` quantiles with Huber threshold ``kappa`` (C
        ABI ``xt_net_set_quant``; ``spec.action_dim`` is actions * quantiles); ``quantiles`` 1 clears the mark.  A net
        carries one mark: ``set_dist`` and this refuse a net the other has marked."""
        L.check(self.lib.xt_net_set_quant(self.handle, int(quantiles), float(kappa)), "xt_net_set_quant")
        self.quant = (int(quantiles), float(kappa)) if int(quantiles) > 1 else None
        if self.quant is None:
            self.duel = False                           # (clearing the mark clears the dueling one)

    def set_duel(self, on):
        """Mark a net that carries the mark of ``set_dist`` / ``set_quant`` as dueling (C ABI ``xt_net_set_duel``): the last
        group of its head is the state-value stream (``netspec`` with ``dist_dueling``), and ``dqn_step`` with ``dist`` /
        ``quant`` runs the dueling head.  Clearing the other mark clears this one."""
        L.check(self.lib.xt_net_set_duel(self.handle, int(bool(on))), "xt_net_set_duel")
        self.duel = bool(on)

    def set_noisy(self, seed, sigma0):
        """Give the noisy layers of the net's spec the 64-bit key ``seed`` of their noise draws; ``sigma0`` is the spec's
        (what ``initial_weights`` started the sigmas from) and is only checked.  A plain spec is refused."""
        if self.params_eff is None:
            raise ValueError("set_noisy: the net's spec has no noisy layers (netspec.dqn_cnn / dqn_mlp with noisy=True)")
        if float(sigma0) != self.spec.noisy_sigma0:
            raise ValueError("set_noisy: sigma0 = {} differs from the spec's noisy_sigma0 = {}".format(
                sigma0, self.spec.noisy_sigma0))
        self.noisy = (int(seed) & 0xFFFFFFFFFFFFFFFF, float(sigma0))

    def compose(self, call, stream_id, mean_only=False, noise_in=None):
        """The effective parameters of the net for its next forward / step (C ABI ``xt_noisy_compose``, one launch, nothing
        synchronises): W_eff = mu + sigma * (f_in f_out^T) over the noisy layers with the vectors of (seed, ``call``,
        ``stream_id``), which stay in ``self.noise``; every other parameter is copied.  ``mean_only``: W_eff = mu.
        ``noise_in`` (float32 device tensor laid out as ``self.noise``): the vectors are taken from it instead of drawn."""
        if getattr(self, "noisy", None) is None:
            raise ValueError("compose: the net has no noise key (call set_noisy first)")
        L.check(self.lib.xt_noisy_compose(
            self._noisy_table, len(self._noisy_table), L.ptr(self.params), L.ptr(self.params_eff), self.spec.n_net,
            L.ptr(self.noise), L.ptr(noise_in), self.noisy[0], int(call) & 0xFFFFFFFFFFFFFFFF, int(stream_id),
            1 if mean_only else 0, L.stream_ptr()), "xt_noisy_compose")

    def noisy_grads(self):
        """Behind a step: the sigma blocks of ``self.grads`` = dW_eff * e / db_eff * f_out, from grads[0, n_net) and the vectors
        the last ``compose`` stored (C ABI ``xt_noisy_grads``, one launch)"""
        L.check(self.lib.xt_noisy_grads(self._noisy_table, len(self._noisy_table), L.ptr(self.noise), L.ptr(self.grads),
                                        L.stream_ptr()), "xt_noisy_grads")

    def set_dist_wide(self, on):
        """Switch a marked net between the wide-head kernels (the default) and those of an unmarked net (C ABI
        ``xt_net_set_dist_wide``): for same-run comparisons and tests.  ``on`` = "forward": the wide forward with the generic
        feature-gradient kernel behind it."""
        L.check(self.lib.xt_net_set_dist_wide(self.handle, 2 if on == "forward" else int(bool(on))), "xt_net_set_dist_wide")

    def _nstep_cfg(self, who, follow, n, cap):
        """-> ``NstepCfg`` after the check of ``follow``; allocates the label scratch ``nstep_*`` [max_batch]"""
        if not (follow.is_cuda and follow.is_contiguous() and follow.dtype == torch.int32 and follow.shape[0] == cap):
            raise ValueError("{}: follow must be a contiguous int32 device tensor ({} rows)".format(who, cap))
        if not hasattr(self, "nstep_boot"):
            new = lambda dt: torch.zeros(self.max_batch, dtype=dt, device=self.device)
            self.nstep_boot, self.nstep_action = new(torch.int32), new(torch.int32)
            self.nstep_reward, self.nstep_disc, self.nstep_done = new(torch.float64), new(torch.float64), new(torch.uint8)
        return L.NstepCfg(int(n), follow.data_ptr(), self.nstep_boot.data_ptr(), self.nstep_action.data_ptr(),
                          self.nstep_reward.data_ptr(), self.nstep_disc.data_ptr(), self.nstep_done.data_ptr())

    def apply(self, lr, clip_norm, grad_scale=1.0):
        self.touch()
        L.check(self.lib.xt_net_apply(self.handle, lr, 0.9, 0.999, 1e-8, clip_norm, grad_scale, L.stream_ptr()),
                "xt_net_apply")

    def layer_buffers(self, layer, b):
        """(activation, d-pre-activation) views of the workspace for the first ``b`` samples of ``layer`` (tests)."""
        off = (ctypes.c_int64 * 4)()
        L.check(self.lib.xt_net_layer_offsets(self.handle, layer, off), "xt_net_layer_offsets")
        lay = self.spec.layers[layer]
        n = b * lay.OH * lay.OW * lay.N
        return self.workspace[off[0]:off[0] + n], self.workspace[off[1]:off[1] + n]

    def time_layer(self, layer, which, obs, idx, b, reps=20):
        ms = ctypes.c_float()
        L.check(self.lib.xt_net_time_layer(self.handle, layer, which, L.ptr(obs), L.ptr(idx), b, reps,
                                           ctypes.byref(ms), L.stream_ptr()), "xt_net_time_layer")
        return ms.value

    def time_tail(self, lr=2.5e-4, clip_norm=5.0, reps=50):
        """average ms of the step's tail (gradient reduction, [exchange], clip + Adam) in the net's current mode, on the
        slabs of the most recent gradient step (C ABI xt_net_time_tail)"""
        ms = ctypes.c_float()
        self.touch()
        L.check(self.lib.xt_net_time_tail(self.handle, float(lr), float(clip_norm), int(reps), ctypes.byref(ms),
                                          L.stream_ptr()), "xt_net_time_tail")
        return ms.value

    def grads_dict(self):
        flat = self.grads.detach().cpu().numpy()
        out = OrderedDict()
        for name in self.spec.names:
            out[name] = self.spec.var_view(flat, name).copy()
        return out
