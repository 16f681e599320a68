"""``ImpalaCnn`` / ``ImpalaMlp``: the models of the non-opt ``IMPALA`` algorithm on HIP kernels.

Reference: Keras models with a SOFTMAX policy output and a value output, trained by ``model.fit`` (one epoch,
minibatches of 128, shuffled) on the custom ``impala_loss`` + 0.5 * mse with ``tf.keras`` Adam
(xt/model/impala/impala_cnn.py:33-108: ``clipnorm=40.``, ``decay=5.12e-9``; xt/model/impala/impala_mlp.py:30-93: plain
Adam).  ``predict([state, adv])`` returns ``[probabilities, value [N,1]]``; ``train([state, adv], [one-hot, target])``
returns the epoch's sample-weighted mean loss (what ``History.history['loss'][0]`` holds there).
"""
import numpy as np
import torch

from xingtian_amd.model import netspec
from xingtian_amd.model.hip_net import keras_fit_table
from xingtian_amd.model.impala.default_config import ENTROPY_LOSS, HIDDEN_SIZE, LR, NUM_LAYERS  # noqa: F401
from xingtian_amd.model.model import XTModel, as_numpy, build_net
from xingtian_amd.register import Registers, import_config

FIT_BATCH = 128     # model.fit(batch_size=128), impala_cnn.py:76-80 / impala_mlp.py:68-72


class _KerasImpalaModel(XTModel):
    CLIPNORM, DECAY = 0.0, 0.0

    def __init__(self, model_info):
        model_config = model_info.get("model_config") or {}
        import_config(globals(), model_config)
        self.state_dim, self.action_dim = model_info["state_dim"], model_info["action_dim"]
        self.seed = model_config.get("SEED")
        # forward batches of the algorithm's pre-training pass over all stored states; a fit minibatch is 128 rows
        self.max_batch = max(FIT_BATCH, int(model_config.get("MAX_BATCH", model_info.get("max_batch", 1024))))
        self.iterations = 0                       # optimizer.iterations of tf.keras Adam
        super().__init__(model_info)

    def _spec(self):
        raise NotImplementedError

    def create_model(self, model_info):
        self.net = build_net(model_info, self._spec(), self.max_batch, self.seed)
        self.actor_var = self.net
        if self.net.inference_only:
            return True
        self._acc = torch.zeros((2,), dtype=torch.float32, device=self.net.device)
        return True

    def extra_optimizer_state(self):
        return {"keras_adam_iterations": np.int64(self.iterations)}

    def restore_extra_optimizer_state(self, arrays):
        if "keras_adam_iterations" in arrays:
            self.iterations = int(arrays["keras_adam_iterations"])

    def predict(self, state):
        """-> [softmax probabilities [N,A], value [N,1]] (numpy float32); ``state`` = [observations, dummy adv]."""
        logits, value = self.net.forward(np.asarray(state[0]))
        logits = torch.as_tensor(as_numpy(logits)) if self.net.inference_only else logits
        return [as_numpy(torch.softmax(logits, dim=-1)), as_numpy(value).reshape(-1, 1)]

    def train(self, state, label):
        obs, adv = state
        onehot, target = label
        n = len(obs)
        order = np.arange(n)
        np.random.shuffle(order)                  # model.fit(shuffle=True) draws from numpy's global generator
        return self.fit_in_order(obs, adv, onehot, target, order)

    def fit_in_order(self, obs, adv, onehot, target, order):
        """One epoch over the minibatches ``order[0:128], order[128:256], ...`` (the permutation injected)."""
        self._require_learner()
        dev = self.net.device
        up = lambda a: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float32))).to(dev)
        d_obs = self.net.to_device_obs(obs)
        d_adv, d_hot, d_tgt = up(np.asarray(adv).reshape(-1)), up(onehot), up(np.asarray(target).reshape(-1))
        d_order = torch.from_numpy(np.ascontiguousarray(order, dtype=np.int32)).to(dev)
        self._acc.zero_()
        for lo in range(0, len(order), FIT_BATCH):
            self.net.keras_impala_step(d_obs, d_order[lo:lo + FIT_BATCH], d_adv, d_hot, d_tgt, ENTROPY_LOSS, self._acc)
            self.net.adam_keras(LR, self.iterations, clipnorm=self.CLIPNORM, decay=self.DECAY)
            self.iterations += 1
        acc = self._acc.cpu().numpy()
        return float(acc[0] / acc[1])

    def train_fragments(self, states, onehot, behaviour, reward, done, episode_len, gamma, batch_size, orders=None):
        """One whole ``IMPALA.train`` on the device (``HipActorCritic.keras_impala_train``): the forward over all stored
        states, the float64 v-trace and every fit minibatch are enqueued by ONE C call; the observations are uploaded
        once and the host reads back only the per-chunk loss sums.

        ``states`` [F * (episode_len + 1), ...]; ``onehot`` / ``behaviour`` [F * episode_len, A]; ``reward`` / ``done``
        [F * episode_len(, 1)].  ``batch_size`` is the algorithm's BATCH_SIZE (one ``model.fit`` per sequential chunk of
        transitions); ``orders`` injects the per-chunk permutations, else they are drawn as ``train`` draws them.
        Returns the mean over chunks of the epoch losses (``np.mean`` of what the chunk-wise ``train`` calls return).
        The device buffers of the call stay in ``self.last_fragments`` (tests read ``pg_adv`` / ``target`` there)."""
        self._require_learner()
        t, a = int(episode_len), self.action_dim
        n = len(onehot)
        frags = n // t
        if n == 0 or frags * t != n or len(states) != frags * (t + 1):
            raise ValueError("train_fragments: {} transitions / {} states are not whole fragments of {} (+1) steps".format(
                n, len(states), t))
        orders = draw_fit_orders(n, batch_size) if orders is None else [np.asarray(o) for o in orders]
        bounds = list(range(0, n, batch_size))
        if len(orders) != len(bounds) or any(not np.array_equal(np.sort(o), np.arange(min(batch_size, n - lo)))
                                             for o, lo in zip(orders, bounds)):
            raise ValueError("train_fragments: orders must hold one permutation per BATCH_SIZE chunk")
        # transition i of the flat [F * T] order sits in observation row (i // T) * (T + 1) + i % T
        flat = np.concatenate([lo + o for o, lo in zip(orders, bounds)]).astype(np.int64)
        idx = ((flat // t) * (t + 1) + flat % t).astype(np.int32)
        dev = self.net.device

        def rows(x, dtype, width):
            """[F * T, width] host array -> [F * (T + 1), width] device tensor, slot T of every fragment zero"""
            out = np.zeros((frags, t + 1, width), dtype=dtype)
            out[:, :t] = np.asarray(x).reshape(frags, t, width)
            return torch.from_numpy(out.reshape((frags * (t + 1), width) if width > 1 else (frags * (t + 1),))).to(dev)

        table = keras_fit_table(n, batch_size, FIT_BATCH, self.iterations, LR, self.DECAY)
        out = self.net.keras_impala_train(
            self.net.to_device_obs(states), frags, t, rows(onehot, np.float32, a), rows(behaviour, np.float32, a),
            rows(reward, np.float64, 1), rows(done, np.uint8, 1), torch.from_numpy(idx).to(dev), table, gamma,
            ENTROPY_LOSS, clipnorm=self.CLIPNORM)
        self.iterations += len(table)
        self.last_fragments = out
        acc = out["acc"].cpu().numpy()
        return np.mean([float(s / c) for s, c in acc])


def draw_fit_orders(n_rows, batch_size):
    """The shuffles of one ``IMPALA.train`` over ``n_rows`` transitions: one ``model.fit(shuffle=True)`` permutation per
    sequential ``batch_size`` chunk, drawn chunk by chunk from numpy's global generator exactly as
    ``_KerasImpalaModel.train`` draws them."""
    orders = []
    for lo in range(0, n_rows, batch_size):
        order = np.arange(min(batch_size, n_rows - lo))
        np.random.shuffle(order)
        orders.append(order)
    return orders


@Registers.model
class ImpalaCnn(_KerasImpalaModel):
    CLIPNORM, DECAY = 40.0, 0.00000000512

    def _spec(self):
        return netspec.impala_cnn(tuple(self.state_dim), self.action_dim)


@Registers.model
class ImpalaMlp(_KerasImpalaModel):
    def _spec(self):
        return netspec.impala_mlp(tuple(self.state_dim), self.action_dim, HIDDEN_SIZE, NUM_LAYERS)
