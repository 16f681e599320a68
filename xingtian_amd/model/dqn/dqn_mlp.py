"""``DqnMlp``: NUM_LAYERS x Dense(HIDDEN_SIZE, relu) and the Q head(s), plain tf.keras Adam
(xt/model/dqn/dqn_mlp.py:43-58); everything else is ``DqnModel``."""
from xingtian_amd.model import netspec
from xingtian_amd.model.dqn.default_config import HIDDEN_SIZE, LR, NUM_LAYERS  # noqa: F401
from xingtian_amd.model.dqn.dqn_cnn import DqnModel
from xingtian_amd.register import Registers, import_config


@Registers.model
class DqnMlp(DqnModel):
    def __init__(self, model_info):
        import_config(globals(), model_info.get("model_config") or {})
        super().__init__(model_info, LR)

    def _spec(self):
        return netspec.dqn_mlp(tuple(self.state_dim), self.action_dim, HIDDEN_SIZE, NUM_LAYERS, self.dueling,
                               self.atoms, self.quantiles, self.noisy, self.noisy_sigma0, self.dist_dueling)
