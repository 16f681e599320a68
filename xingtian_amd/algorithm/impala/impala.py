"""``IMPALA`` (the non-"Opt" form): v-trace on the host, in numpy, from the actor's own forward pass.

Reference behaviour (xt/algorithm/impala/impala.py:31-190): every rollout fragment carries ``episode_len + 1`` states
but ``episode_len`` transitions (one-hot ``real_action``, reward, done, and the behaviour policy's action
PROBABILITIES in ``action``).  ``train`` runs the current model over all stored states, forms truncated importance
weights rho = min(1, pi(a|s)/mu(a|s)) from probabilities with ``log(p + 1e-10)``, accumulates the v-trace correction
backwards with the convention  acc[j] += acc[j+1] * discount[j+1] * rho[j+1]  (the "Opt" graph uses discount[j] *
c[j], xt/model/impala/vtrace.py:94-96 -- the two are NOT the same recursion), and hands
(state, pg_advantage) / (one-hot action, v-trace target) to ``Model.train`` in sequential BATCH_SIZE chunks.
Everything is float64 on the host except what the model returns; the model (``ImpalaCnn`` / ``ImpalaMlp``) runs the
forward and the update on the GPU.

Opt-in (``alg_config: {DEVICE_VTRACE: true}``, default off) ``train`` hands the stacked fragments to the model's
``train_fragments`` instead: forward, the same recursion as a float64 kernel (``xt_vtrace_probs_f64``, rho from a
float64 softmax of the logits) and every fit minibatch in one device-resident pass.
"""
import os

import numpy as np

from xingtian_amd.algorithm.algorithm import Algorithm, RolloutFields
from xingtian_amd.algorithm.alg_utils import FIFODistPolicy
from xingtian_amd.algorithm.impala.default_config import BATCH_SIZE, GAMMA
from xingtian_amd.register import Registers, import_config

LOG_EPS = 1e-10
DEVICE_MAX_T, DEVICE_MAX_A = 1024, 64     # limits of the device v-trace kernel (xt_vtrace_probs_f64)


def chosen_logp(prob, onehot):
    """log(sum_a prob*onehot + 1e-10): log-probability of the taken action from a probability vector."""
    return np.log((prob * onehot).sum(axis=-1) + LOG_EPS)


def vtrace_from_probs(target_prob, behaviour_prob, onehot, reward, done, value, value_next, gamma):
    """Host v-trace of the reference (impala.py:139-167) for fragments shaped [n_fragments, T, ...].

    target_prob / behaviour_prob / onehot: [F, T, A]; reward / done: [F, T, 1]; value / value_next: [F, T, 1]
    (V(s_t) and V(s_{t+1})).  Returns (pg_advantage, vtrace_target), both [F, T, 1] float64.
    """
    return vtrace_from_rho(rho_from_probs(target_prob, behaviour_prob, onehot), reward, done, value, value_next, gamma)


def rho_from_probs(target_prob, behaviour_prob, onehot):
    """Truncated importance weights min(1, pi(a|s) / mu(a|s)) of the taken actions, [F, T, 1]."""
    return np.minimum(np.exp(chosen_logp(target_prob, onehot) - chosen_logp(behaviour_prob, onehot)), 1.0)[..., None]


def vtrace_from_rho(rho, reward, done, value, value_next, gamma):
    """The recursion of ``vtrace_from_probs`` on given importance weights ``rho`` [F, T, 1] (what the device kernel
    ``xt_vtrace_probs_f64`` evaluates with the same roundings).  Returns (pg_advantage, vtrace_target)."""
    discount = np.logical_not(done) * gamma
    acc = rho * (reward + discount * value_next - value)          # per-step corrected TD errors
    for j in reversed(range(acc.shape[1] - 1)):                   # suffix accumulation, reference index convention
        acc[:, j] += acc[:, j + 1] * discount[:, j + 1] * rho[:, j + 1]
    target = value + acc
    target_next = np.concatenate([target[:, 1:], value_next[:, -1:]], axis=1)   # bootstrap with V of the last state
    pg_adv = rho * (reward + discount * target_next - value)
    return pg_adv, target


@Registers.algorithm
class IMPALA(Algorithm):
    FIELDS = ("cur_state", "real_action", "done", "action", "reward")

    def __init__(self, model_info, alg_config, **kwargs):
        import_config(globals(), alg_config)
        actor_info = dict(model_info["actor"])
        super().__init__(alg_name="impala", model_info=actor_info, alg_config=alg_config)
        self.dummy_action, self.dummy_value = np.zeros((1, self.action_dim)), np.zeros((1, 1))
        self.async_flag = False
        self.episode_len = alg_config.get("episode_len", 128)
        self._rollout = RolloutFields(*self.FIELDS)
        self.dist_model_policy = FIFODistPolicy(alg_config["instance_num"], prepare_times=self._prepare_times_per_train)

    # list-per-field names of the reference (impala.py:54-59)
    state = property(lambda self: self._rollout.parts["cur_state"])
    action = property(lambda self: self._rollout.parts["real_action"])
    dones = property(lambda self: self._rollout.parts["done"])
    pred_a = property(lambda self: self._rollout.parts["action"])
    rewards = property(lambda self: self._rollout.parts["reward"])

    @staticmethod
    def _data_proc(episode_data):
        """-> (states, one-hot actions, dones [T,1], behaviour probabilities, rewards [T,1])."""
        column = lambda x: np.asarray(x).reshape(-1, 1)
        return (episode_data["cur_state"], episode_data["real_action"], column(episode_data["done"]),
                np.asarray(episode_data["action"]), column(episode_data["reward"]))

    def prepare_data(self, train_data, **kwargs):
        states, onehot, dones, behaviour, rewards = self._data_proc(train_data)
        self._rollout.add(cur_state=states, real_action=onehot, done=dones, action=behaviour, reward=rewards)

    def _train_proc(self):
        states, onehot, dones, behaviour, rewards = self._rollout.stacked()
        t, s = self.episode_len, self.episode_len + 1
        prob, value = self.actor.predict([states, np.zeros((states.shape[0], 1))])[:2]
        frag = lambda x, step: x.reshape((x.shape[0] // step, step) + x.shape[1:])
        prob, value = frag(prob, s), frag(value, s)
        onehot_f = frag(onehot, t)
        pg_adv, target = vtrace_from_probs(prob[:, :-1], frag(behaviour, t), onehot_f, frag(rewards, t),
                                           frag(dones, t), value[:, :-1], value[:, 1:], GAMMA)
        flat = lambda x: x.reshape((-1,) + x.shape[2:])
        return flat(frag(states, s)[:, :-1]), flat(pg_adv), flat(target), flat(onehot_f)

    def _device_train_ok(self):
        """``DEVICE_VTRACE`` (default off): forward, v-trace and every fit minibatch in one device-resident pass
        (``_KerasImpalaModel.train_fragments``), where the actor has it and the v-trace kernel holds the fragment."""
        return (bool(self.alg_config.get("DEVICE_VTRACE", False)) and hasattr(self.actor, "train_fragments")
                and self.episode_len <= DEVICE_MAX_T and self.action_dim <= DEVICE_MAX_A)

    def train(self, **kwargs):
        if self._device_train_ok():
            states, onehot, dones, behaviour, rewards = self._rollout.stacked()
            loss = self.actor.train_fragments(states, onehot, behaviour, rewards, dones, self.episode_len, GAMMA,
                                              BATCH_SIZE)
            self._rollout.reset()
            return loss
        states, pg_adv, target, onehot = self._train_proc()
        losses = []
        for lo in range(0, len(states), BATCH_SIZE):
            hi = lo + BATCH_SIZE
            losses.append(self.actor.train([states[lo:hi], pg_adv[lo:hi]], [onehot[lo:hi], target[lo:hi]]))
        self._rollout.reset()
        return np.mean(losses)

    def predict(self, state):
        return self.actor.predict([state.reshape((1,) + state.shape), np.zeros((1, 1))])

    def save(self, model_path, model_index):
        saved = self.actor.save_model(os.path.join(model_path, "actor" + str(model_index).zfill(5)))
        return [saved.split("/")[-1]]
