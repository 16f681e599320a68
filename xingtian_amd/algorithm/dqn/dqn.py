"""``DQN``: deep Q-learning with a replay store that lives on the device.

Reference behaviour (xt/algorithm/dqn/dqn.py:36-148, xt/algorithm/replay_buffer.py): ``prepare_data`` appends the
``len(train_data["done"])`` transitions of a message to a ``deque(maxlen=BUFFER_SIZE)``; ``train`` draws
``min(size, BATCH_SIZE)`` of them with ``random.sample``, bootstraps with ``a* = argmax_a Q_target(next)``
(``double_dqn``: ``argmax_a Q_online(next)``), ``y = done ? r : r + GAMMA * Q_target(next)[a*]``, fits the taken column
of the online network's own prediction to ``y`` (Keras 'mse') and copies the online weights to the target network
every ``TARGET_UPDATE_FREQ``-th train.

Here the deque is five rings in HBM (``DeviceReplay``: state, next state, action, reward, done); a train uploads the
sampled slots (a few hundred bytes) and ONE C call gathers the minibatch, runs both networks, the TD / MSE head and the
backward pass (``xt_net_dqn_step``), followed by tf.keras Adam (``xt_adam_keras``).  The target sync is one
device-to-device copy of the flat parameter buffer.

A model without the device step (anything that only implements the reference's ``predict`` / ``train(states, y_t)``)
is driven the reference's way on the host (``_train_host``), with ``td_targets`` as the arithmetic.

``alg_config.prioritized_replay`` (off unless asked for) swaps the uniform draw for proportional prioritised replay
(xt/algorithm/prioritized_replay_buffer_muzero.py, the baselines form): ``PrioritizedDeviceReplay`` keeps the sum tree,
the min tree and the running maximum priority next to the rings, a train uploads its ``random.random()`` draws and ONE C
call (``xt_net_dqn_step_per``) samples, weights the head and writes the new priorities back.  It needs the device step.

``alg_config.n_step`` (1 unless asked for) trains on n-step returns: the reference's agents send one-step transitions, but
a message holds consecutive steps of one agent and ``DeviceReplay.add`` writes it to contiguous slots, so the rows that
follow a sampled row are next to it in the rings.  A sixth ring, ``follow``, says how many rows come after each slot in
its message; ``nstep_targets`` is the definition, ``xt_net_dqn_step_n`` evaluates it inside the next-state gather.

``model_config.atoms`` > 1 on the actor makes the pair distributional (C51): the train is ``xt_net_dqn_step_dist``, whose
head projects the target distribution of the bootstrap action onto the support and takes the cross-entropy of the taken
action's distribution (``dist_support`` / ``dist_q`` / ``categorical_projection`` are the host definitions).  It composes
with ``double_dqn``, ``prioritized_replay`` (the new priority is the sample's loss + eps) and ``n_step``, and like
prioritised replay it needs the device step.

``model_config.quantiles`` > 1 makes the pair quantile-regression (QR-DQN) instead: the train is
``xt_net_dqn_step_quant``, whose head takes the pairwise quantile-Huber loss between the taken action's quantiles and the
Bellman targets of the bootstrap action's (``quantile_midpoints`` / ``quant_q`` / ``quantile_huber`` are the host
definitions).  There is no support to choose; it composes and is bound to the device step in the same way.

``model_config.noisy`` gives the actor pair factorised-Gaussian noisy layers (NoisyNet): the last trunk layer, the Q head
and the dueling stream run on ``W_eff = mu + sigma * (f_in f_out^T)``, composed on the device in front of every train
(``xt_noisy_compose``, the online net on noise stream 0 and the target net on stream 1 of the call ``iterations``), with
the sigma gradients formed behind it (``xt_noisy_grads``); it composes with everything above, because no step entry
knows about it.  The target sync copies the whole store, means and sigmas.

Every variant reaches its C entry through the model's ``train_replay`` / ``train_replay_per`` and one method of the net,
``HipActorCritic.dqn_step``, whose keywords (``follow`` / ``n``, ``per``, ``dist``, ``quant``) choose the entry.
``model_config.dist_dueling`` with either distributional head makes the network dueling (the value stream folded into the Q
head, ``xt_net_set_duel``): the same two entries read the mark, and nothing changes here.
"""
import random

import numpy as np
import torch

from xingtian_amd.algorithm.algorithm import Algorithm
from xingtian_amd.algorithm.dqn.default_config import BATCH_SIZE, BUFFER_SIZE, GAMMA, TARGET_UPDATE_FREQ
from xingtian_amd.model.dqn.dqn_cnn import categorical_projection, dist_q, dist_support  # noqa: F401
from xingtian_amd.model.dqn.dqn_cnn import quant_q, quantile_huber, quantile_midpoints  # noqa: F401
from xingtian_amd.register import Registers, import_config


def td_targets(reward, done, maxq, gamma):
    """y = done ? r : r + gamma * maxq as the reference's loop evaluates it under NumPy 1.x: the reward is a float64
    scalar, ``gamma * maxq`` promotes the float32 Q value to float64, and storing into the float32 prediction rounds
    once.  ``done`` is truthiness."""
    r = np.asarray(reward, np.float64).reshape(-1)
    g = np.asarray(gamma, np.float64)                  # a scalar, or the per-sample discount of n-step targets
    boot = r + (g.reshape(-1) if g.ndim else float(g)) * np.asarray(maxq, np.float32).reshape(-1).astype(np.float64)
    return np.where(np.asarray(done).reshape(-1).astype(bool), r, boot).astype(np.float32)


def nstep_targets(slots, follow, action, reward, done, gamma, n, capacity):
    """The n-step walk of every start slot in ``slots`` over the label rings (host arrays of ``capacity`` entries), in
    Python floats (IEEE float64, one rounding per operation):

        R = reward[s]; g = gamma; j = s; k = 0
        while k < n - 1 and k < follow[s] and not done[j]:
            k += 1; j = (s + k) % capacity; R = R + g * reward[j]; g = g * gamma

    -> (boot_slot int32, action_n int32, reward_n float64, disc_n float64, done_n uint8), one entry per start slot:
    ``j``, ``action[s]``, ``R``, ``g``, ``done[j]``.  ``y = done_n ? R : R + disc_n * max Q(next_state[boot_slot])``.
    n = 1 is ``(s, action[s], reward[s], gamma, done[s])``.  ``follow[s]`` is the number of rows behind ``s`` in its
    message (negative: 0), so a walk ends with its message.  A start slot outside [0, capacity) reads nothing:
    ``(s, 0, 0.0, gamma, 1)``."""
    n, cap, gamma = int(n), int(capacity), float(gamma)
    if not 1 <= n <= 256:
        raise ValueError("nstep_targets: n = {} outside [1, 256]".format(n))
    out = ([], [], [], [], [])
    for s in (int(x) for x in np.asarray(slots).reshape(-1)):
        if not 0 <= s < cap:
            row = (s, 0, 0.0, gamma, 1)
        else:
            R, g, j, k = float(reward[s]), gamma, s, 0
            while k < n - 1 and k < int(follow[s]) and not done[j]:
                k += 1
                j = (s + k) % cap
                prod = g * float(reward[j])
                R = R + prod
                g = g * gamma
            row = (j, int(action[s]), R, g, int(done[j]))
        for col, x in zip(out, row):
            col.append(x)
    return tuple(np.asarray(col, dt) for col, dt in zip(out, (np.int32, np.int32, np.float64, np.float64, np.uint8)))


class DeviceReplay(object):
    """``ReplayBuffer`` (a ``deque(maxlen=capacity)`` of transitions) as five rings on ``device``: ``cur_state`` /
    ``next_state`` [capacity, ...] in the form the first layer reads (``to_rows``: ``HipActorCritic.to_device_obs``),
    ``action`` int32, ``reward`` float64, ``done`` uint8 [capacity].  Logical index i (0 = oldest) lives in slot
    ``(head + i) % capacity``.  The rings are allocated at the first ``add``.  ``n_step`` > 1 adds a sixth ring, ``follow``
    int32 [capacity]: the number of rows that come after the slot in the message that wrote it."""

    def __init__(self, capacity, device="cpu", to_rows=None, n_step=1):
        if int(capacity) < 1:
            raise ValueError("DeviceReplay: capacity must be positive, got {}".format(capacity))
        self.capacity, self.device = int(capacity), torch.device(device)
        self.n_step = int(n_step)
        self.follow = None
        self._label_bytes = 4 + 8 + 1 + (4 if self.n_step > 1 else 0)
        self._to_rows = to_rows
        self.head = self._size = 0
        self.cur_state = self.next_state = self.action = self.reward = self.done = None

    def size(self):
        return self._size

    def _rows(self, states):
        if self._to_rows is not None:
            return self._to_rows(np.asarray(states))
        return torch.as_tensor(np.ascontiguousarray(states)).to(self.device)

    def _allocate(self, state_rows):
        row_shape, dtype = tuple(state_rows.shape[1:]), state_rows.dtype
        row_bytes = int(np.prod(row_shape, dtype=np.int64)) * state_rows.element_size()
        need = self.capacity * (2 * row_bytes + self._label_bytes)
        if self.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self.device)
            if need > free:
                raise RuntimeError("DeviceReplay: the rings of {} transitions need {} bytes of device memory ({} bytes per "
                                   "state row), {} bytes are free -- lower BUFFER_SIZE".format(
                                       self.capacity, need, row_bytes, free))
        new = lambda shape, dt: torch.empty((self.capacity,) + shape, dtype=dt, device=self.device)
        self.cur_state, self.next_state = new(row_shape, dtype), new(row_shape, dtype)
        self.action, self.reward, self.done = new((), torch.int32), new((), torch.float64), new((), torch.uint8)
        if self.n_step > 1:
            self.follow = torch.zeros(self.capacity, dtype=torch.int32, device=self.device)
        self.bytes = need

    def add(self, cur_state, next_state, action, reward, done):
        """Append the ``len(done)`` transitions of one message, evicting the oldest beyond the capacity: at most two
        contiguous spans per ring.  Of a message longer than the capacity the last ``capacity`` rows stay."""
        n = len(done)
        if n == 0:
            return
        skip = max(0, n - self.capacity)
        host = lambda x, dt: torch.from_numpy(np.ascontiguousarray(np.asarray(x)[skip:].reshape(n - skip), dtype=dt))
        cols = [self._rows(np.asarray(cur_state)[skip:]), self._rows(np.asarray(next_state)[skip:]),
                host(action, np.int32).to(self.device), host(reward, np.float64).to(self.device),
                host(np.asarray(done).astype(bool), np.uint8).to(self.device)]
        if self.cur_state is None:
            self._allocate(cols[0])
        m, cap = n - skip, self.capacity
        w = (self.head + self._size + skip) % cap
        first = min(m, cap - w)
        rings = [self.cur_state, self.next_state, self.action, self.reward, self.done]
        if self.follow is not None:                     # m - 1, m - 2, ... 0 over the rows kept
            rings.append(self.follow)
            cols.append(torch.arange(m - 1, -1, -1, dtype=torch.int32).to(self.device))
        for ring, rows in zip(rings, cols):
            ring[w:w + first] = rows[:first]
            if m > first:
                ring[:m - first] = rows[first:]
        total = self._size + n
        if total > cap:
            self.head, self._size = (self.head + total - cap) % cap, cap
        else:
            self._size = total

    def slots_of(self, logical):
        return [(self.head + int(i)) % self.capacity for i in logical]

    def sample(self, k):
        """The slots of ``random.sample(deque, k)``: the same draw from the global generator over the logical indices."""
        return self.slots_of(random.sample(range(self._size), int(k)))


class PrioritizedDeviceReplay(DeviceReplay):
    """``DeviceReplay`` plus the two segment trees of ``PrioritizedReplayBuffer(capacity, alpha)`` on the device: float64
    ``sum_tree`` / ``min_tree`` [2 * cap2] (cap2: the smallest power of two >= capacity; leaf ``cap2 + slot`` is ring slot
    ``slot``, the reference's ``_next_idx`` being the ring's write position) and ``max_prio`` [1], 1.0 at the start.  Every
    slot a message writes takes the priority ``max_prio ** alpha`` (``xt_per_add``, one call per contiguous span).  The
    trees are allocated with the rings; sampling and the priority update belong to the train (``xt_net_dqn_step_per``)."""

    def __init__(self, capacity, device, to_rows=None, alpha=0.6, eps=1e-6, n_step=1):
        super().__init__(capacity, device, to_rows, n_step)
        if not float(alpha) >= 0.0 or not float(eps) > 0.0:
            raise ValueError("PrioritizedDeviceReplay: alpha = {} must be >= 0 and eps = {} > 0".format(alpha, eps))
        self.alpha, self.eps = float(alpha), float(eps)
        self.cap2 = 1
        while self.cap2 < self.capacity:
            self.cap2 *= 2
        self.sum_tree = self.min_tree = self.max_prio = None

    def _allocate(self, state_rows):
        if self.device.type != "cuda":
            raise NotImplementedError("PrioritizedDeviceReplay: the trees live on the GPU; there is no host form")
        tree_bytes = 2 * 2 * self.cap2 * 8
        free, _ = torch.cuda.mem_get_info(self.device)
        row_bytes = int(np.prod(tuple(state_rows.shape[1:]), dtype=np.int64)) * state_rows.element_size()
        need = self.capacity * (2 * row_bytes + self._label_bytes) + tree_bytes
        if need > free:
            raise RuntimeError("PrioritizedDeviceReplay: the rings of {} transitions and the two priority trees need {} bytes "
                               "of device memory ({} bytes per state row, {} bytes of trees), {} bytes are free -- lower "
                               "BUFFER_SIZE".format(self.capacity, need, row_bytes, tree_bytes, free))
        super()._allocate(state_rows)
        self.bytes += tree_bytes
        self.sum_tree = torch.zeros(2 * self.cap2, dtype=torch.float64, device=self.device)
        self.min_tree = torch.full((2 * self.cap2,), float("inf"), dtype=torch.float64, device=self.device)
        self.max_prio = torch.ones(1, dtype=torch.float64, device=self.device)

    def add(self, cur_state, next_state, action, reward, done):
        n = len(done)
        if n == 0:
            return
        m = min(n, self.capacity)
        w = (self.head + self._size + n - m) % self.capacity        # where DeviceReplay.add starts to write
        super().add(cur_state, next_state, action, reward, done)
        from xingtian_amd import lib as L
        first = min(m, self.capacity - w)
        for start, count in ((w, first), (0, m - first)):
            if count > 0:
                L.check(L.load().xt_per_add(L.ptr(self.sum_tree), L.ptr(self.min_tree), self.cap2, L.ptr(self.max_prio),
                                            start, count, self.alpha, L.stream_ptr()), "xt_per_add")


@Registers.algorithm
class DQN(Algorithm):
    def __init__(self, model_info, alg_config, **kwargs):
        import_config(globals(), alg_config)
        from xingtian_amd.model import model_builder
        actor_info = dict(model_info["actor"])
        actor_info.setdefault("max_batch", int(BATCH_SIZE))
        super().__init__(alg_name="dqn", model_info=actor_info, alg_config=alg_config)
        self.target_actor = model_builder(actor_info)
        self.double_dqn = alg_config.get("double_dqn", False)
        net = getattr(self.actor, "net", None)
        self.device_step = hasattr(self.actor, "train_replay") and not getattr(net, "inference_only", True)
        self.atoms = int(getattr(self.actor, "atoms", 1))
        if self.atoms > 1 and not self.device_step:
            raise NotImplementedError(
                "DQN: a distributional actor (atoms = {}) needs a model with the device step (a learner DqnCnn / DqnMlp on "
                "the GPU): the target distribution is projected on the device, where the target network's output is; {} "
                "has none".format(self.atoms, type(self.actor).__name__))
        self.quantiles = int(getattr(self.actor, "quantiles", 1))
        if self.quantiles > 1 and not self.device_step:
            raise NotImplementedError(
                "DQN: a quantile actor (quantiles = {}) needs a model with the device step (a learner DqnCnn / DqnMlp on "
                "the GPU): the quantile targets are formed on the device, where the target network's output is; {} "
                "has none".format(self.quantiles, type(self.actor).__name__))
        self.prioritized = bool(alg_config.get("prioritized_replay", False))
        n_step = alg_config.get("n_step", 1)
        if isinstance(n_step, bool) or not isinstance(n_step, (int, np.integer)) or not 1 <= n_step <= 256:
            raise ValueError("DQN: n_step = {!r} must be an integer in [1, 256]".format(n_step))
        self.n_step = int(n_step)
        if self.prioritized:
            if not (self.device_step and hasattr(self.actor, "train_replay_per")):
                raise NotImplementedError(
                    "DQN: prioritized_replay needs a model with the device step (a learner DqnCnn / DqnMlp on the GPU): the "
                    "priority trees live next to the device rings; {} has none".format(type(self.actor).__name__))
            if int(BATCH_SIZE) > 1024:
                raise ValueError("DQN: prioritized_replay samples with one thread per transition in one workgroup: "
                                 "BATCH_SIZE = {} exceeds 1024".format(BATCH_SIZE))
            self.per_beta0 = float(alg_config.get("prioritized_replay_beta0", 0.4))
            self.per_beta_iters = alg_config.get("prioritized_replay_beta_iters", None)
            if not 0.0 < self.per_beta0 <= 1.0:
                raise ValueError("DQN: prioritized_replay_beta0 = {} outside (0, 1]".format(self.per_beta0))
            if self.per_beta_iters is not None and int(self.per_beta_iters) < 1:
                raise ValueError("DQN: prioritized_replay_beta_iters = {} must be positive or None".format(self.per_beta_iters))
            self.buff = PrioritizedDeviceReplay(BUFFER_SIZE, net.device, net.to_device_obs,
                                                alg_config.get("prioritized_replay_alpha", 0.6),
                                                alg_config.get("prioritized_replay_eps", 1e-6), self.n_step)
        elif self.device_step:
            self.buff = DeviceReplay(BUFFER_SIZE, net.device, net.to_device_obs, self.n_step)
        else:
            self.buff = DeviceReplay(BUFFER_SIZE, n_step=self.n_step)

    def prepare_data(self, train_data, **kwargs):
        self.buff.add(train_data["cur_state"], train_data["next_state"], train_data["action"], train_data["reward"],
                      train_data["done"])

    def train(self, **kwargs):
        if self.prioritized:
            return self._train_prioritized()
        return self.train_on_slots(self.buff.sample(min(self.buff.size(), BATCH_SIZE)))

    def per_beta(self):
        """the importance exponent of the next train: constant ``beta0``, or linear from ``beta0`` to 1.0 over
        ``prioritized_replay_beta_iters`` trains (the baselines ``LinearSchedule``)"""
        if self.per_beta_iters is None:
            return self.per_beta0
        frac = min(float(self.train_count) / float(int(self.per_beta_iters)), 1.0)
        return self.per_beta0 + frac * (1.0 - self.per_beta0)

    def _train_prioritized(self):
        """One prioritised train: ``min(size, BATCH_SIZE)`` draws of ``random.random()`` go up, the device samples,
        trains and writes the priorities back.  -> the loss as a float."""
        size = self.buff.size()
        if size < 2:
            raise ValueError("DQN.train: prioritized replay cannot sample from {} stored transition(s): the mass range "
                             "excludes the last stored slot, at least 2 are needed".format(size))
        u = torch.tensor([random.random() for _ in range(min(size, BATCH_SIZE))], dtype=torch.float64).to(self.buff.device)
        out = self.actor.train_replay_per(self.target_actor, self.buff, u, self.per_beta(), GAMMA, self.double_dqn)
        self._count_train()
        return float(out[0].item())

    def train_on_slots(self, slots):
        """One train on the given ring slots (``train`` draws them; tests inject them).  -> the loss as a float."""
        if self.device_step:
            d_slots = torch.tensor(slots, dtype=torch.int32).to(self.buff.device)
            out = self.actor.train_replay(self.target_actor, self.buff, d_slots, GAMMA, self.double_dqn)
            self._count_train()
            return float(out[0].item())
        return self._train_host(slots)

    def _count_train(self):
        """the tail of every train: count it and copy the weights to the target network every ``TARGET_UPDATE_FREQ``-th"""
        self.train_count += 1
        if self.train_count % TARGET_UPDATE_FREQ == 0:
            self.update_target()

    def _train_host(self, slots):
        at = lambda ring, idx=slots: ring[torch.as_tensor(idx, dtype=torch.int64)].cpu().numpy()
        if self.n_step > 1:                             # the labels of the walk; the next states of the boot slots
            host = lambda ring: ring.cpu().numpy()
            boot, action, reward, gamma, done = nstep_targets(
                slots, host(self.buff.follow), host(self.buff.action), host(self.buff.reward), host(self.buff.done), GAMMA,
                self.n_step, self.buff.capacity)
        else:
            boot, action, reward, gamma, done = slots, at(self.buff.action), at(self.buff.reward), GAMMA, at(self.buff.done)
        states, new_states = at(self.buff.cur_state), at(self.buff.next_state, boot)
        y_t = self.actor.predict(states)
        target_q = self.target_actor.predict(new_states)
        pick = np.argmax(self.actor.predict(new_states) if self.double_dqn else target_q, 1)
        rows = np.arange(len(slots))
        y_t[rows, action] = td_targets(reward, done, target_q[rows, pick], gamma)
        loss = self.actor.train(states, y_t)
        self._count_train()
        return loss

    def update_target(self):
        if hasattr(self.target_actor, "copy_weights_from"):
            self.target_actor.copy_weights_from(self.actor)
        else:
            self.target_actor.set_weights(self.actor.get_weights())

    def restore(self, model_name=None, model_weights=None):
        """Both networks take the restored weights (dqn.py:105-119)."""
        if model_weights is not None:
            self.actor.set_weights(model_weights)
            self.target_actor.set_weights(model_weights)
        else:
            self.actor.load_model(model_name)
            self.target_actor.load_model(model_name)
