"""``DqnCnn``: the Q-network of the ``DQN`` algorithm on HIP kernels (base class of ``DqnMlp`` too).

Reference: a Keras model with one linear output Q [N, A] -- with ``model_config.dueling`` the 1-wide stream ``s`` and
the A-wide stream ``l`` combine to Q_a = s + (l_a - mean_a l) -- compiled with ``loss='mse'`` and ``tf.keras`` Adam
(xt/model/dqn/dqn_cnn.py:45-61: ``clipnorm=10.``; xt/model/dqn/dqn_mlp.py:43-58: plain Adam).  ``predict(state)``
returns Q as float32 [N, A].  The update does not go through ``train(states, y_t)``: the algorithm keeps its replay
store on the device and one C call (``xt_net_dqn_step``) forms the TD target and the gradient there
(``train_replay``), so ``train`` is not provided.
"""
import numpy as np

from xingtian_amd.model import netspec
from xingtian_amd.model.dqn.default_config import LR  # noqa: F401
from xingtian_amd.model.model import XTModel, as_numpy, build_net
from xingtian_amd.register import Registers, import_config

PONG_MESSAGE = ("DqnCnnPong is not supported: its input dtype is int8, for which the input transform has no mode "
                "(uint8 and float32 only)")


def dueling_q(logits, value, dueling):
    """Q [N, A] float32 from the two heads: the A-wide head as it is, or s + (l - mean_a l) with the 1-wide head s."""
    l = np.asarray(logits, np.float32)
    if not dueling:
        return l
    return np.asarray(value, np.float32).reshape(-1, 1) + (l - l.mean(axis=1, keepdims=True, dtype=np.float32))


def dqn_spec(model_info):
    """The ``NetSpec`` of a DQN model description (``model_para.actor`` of a YAML): ``DqnCnn`` / ``DqnMlp``."""
    cfg = model_info.get("model_config") or {}
    name, dueling = model_info["model_name"], bool(cfg.get("dueling", False))
    if name == "DqnCnnPong":
        raise NotImplementedError(PONG_MESSAGE)
    if name == "DqnCnn":
        return netspec.dqn_cnn(tuple(model_info["state_dim"]), model_info["action_dim"], dueling)
    if name == "DqnMlp":
        from xingtian_amd.model.dqn import default_config as d
        return netspec.dqn_mlp(tuple(model_info["state_dim"]), model_info["action_dim"],
                               cfg.get("HIDDEN_SIZE", d.HIDDEN_SIZE), cfg.get("NUM_LAYERS", d.NUM_LAYERS), dueling)
    raise KeyError("no DQN model named {}".format(name))


class DqnModel(XTModel):
    CLIPNORM = 0.0

    def __init__(self, model_info, learning_rate):
        model_config = model_info.get("model_config") or {}
        self.state_dim, self.action_dim = model_info["state_dim"], model_info["action_dim"]
        self.learning_rate = learning_rate
        self.dueling = bool(model_config.get("dueling", False))
        self.seed = model_config.get("SEED")
        # the algorithm's minibatch (model_info["max_batch"], set by DQN) bounds the training step; predict walks larger
        # inputs in chunks
        self.max_batch = int(model_config.get("MAX_BATCH", model_info.get("max_batch", 256)))
        self.iterations = 0                       # optimizer.iterations of tf.keras Adam
        super().__init__(model_info)

    def _spec(self):
        raise NotImplementedError

    def create_model(self, model_info):
        self.net = build_net(model_info, self._spec(), self.max_batch, self.seed)
        self.actor_var = self.net
        return True

    def extra_optimizer_state(self):
        return {"keras_adam_iterations": np.int64(self.iterations)}

    def restore_extra_optimizer_state(self, arrays):
        if "keras_adam_iterations" in arrays:
            self.iterations = int(arrays["keras_adam_iterations"])

    def predict(self, state):
        """-> Q [N, A] (numpy float32)"""
        logits, value = self.net.forward(np.asarray(state))
        return dueling_q(as_numpy(logits), as_numpy(value), self.dueling)

    def train_replay(self, target, replay, slots, gamma, double_dqn):
        """One update on the minibatch ``slots`` (int32 device tensor) of the device rings ``replay``
        (``algorithm.dqn.DeviceReplay``): ``xt_net_dqn_step`` with ``target``'s network as the target net, then tf.keras
        Adam.  Nothing synchronises.  -> the device tensor [loss, mean |TD error|, mean bootstrap Q].  A replay with
        ``n_step`` > 1 trains on n-step targets (``xt_net_dqn_step_n``)."""
        self._require_learner()
        if getattr(replay, "n_step", 1) > 1:
            out = self.net.dqn_step_n(target.net, replay.cur_state, replay.next_state, slots, replay.action, replay.reward,
                                      replay.done, replay.follow, replay.n_step, gamma, self.dueling, double_dqn)
        else:
            out = self.net.dqn_step(target.net, replay.cur_state, replay.next_state, slots, replay.action, replay.reward,
                                    replay.done, gamma, self.dueling, double_dqn)
        self.net.adam_keras(self.learning_rate, self.iterations, clipnorm=self.CLIPNORM)
        self.iterations += 1
        return out

    def train_replay_per(self, target, replay, u, beta, gamma, double_dqn):
        """``train_replay`` on a ``PrioritizedDeviceReplay``: the minibatch is drawn on the device with the uniform draws
        ``u`` (float64 device tensor [B]) and importance exponent ``beta``, and the replay's trees take the new TD errors
        (``xt_net_dqn_step_per``), then tf.keras Adam.  Nothing synchronises.  -> the device tensor of ``train_replay``."""
        self._require_learner()
        if getattr(replay, "n_step", 1) > 1:
            per = dict(size=replay.size(), u=u, sum_tree=replay.sum_tree, min_tree=replay.min_tree,
                       max_prio=replay.max_prio, alpha=replay.alpha, beta=beta, eps=replay.eps)
            out = self.net.dqn_step_n(target.net, replay.cur_state, replay.next_state, None, replay.action, replay.reward,
                                      replay.done, replay.follow, replay.n_step, gamma, self.dueling, double_dqn, per=per)
        else:
            out = self.net.dqn_step_per(target.net, replay.cur_state, replay.next_state, replay.size(), u, replay.action,
                                        replay.reward, replay.done, gamma, self.dueling, double_dqn, replay.sum_tree,
                                        replay.min_tree, replay.max_prio, replay.alpha, beta, replay.eps)
        self.net.adam_keras(self.learning_rate, self.iterations, clipnorm=self.CLIPNORM)
        self.iterations += 1
        return out

    def copy_weights_from(self, other):
        """this network's parameters <- ``other``'s: one device-to-device copy of the flat buffer on a learner"""
        if getattr(self.net, "inference_only", False) or getattr(other.net, "inference_only", False):
            self.set_weights(other.get_weights())
            return
        self.net.params.copy_(other.net.params)
        self.net.touch()


@Registers.model
class DqnCnn(DqnModel):
    CLIPNORM = 10.0

    def __init__(self, model_info):
        import_config(globals(), model_info.get("model_config") or {})
        super().__init__(model_info, LR)

    def _spec(self):
        return netspec.dqn_cnn(tuple(self.state_dim), self.action_dim, self.dueling)
