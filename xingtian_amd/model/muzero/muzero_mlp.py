"""``MuzeroMlp`` (xt/model/muzero/muzero_mlp.py): Dense HIDDEN1_UNITS -> HIDDEN2_UNITS representation, hidden width
HIDDEN2_UNITS; see ``muzero_model``."""
from xingtian_amd.model.muzero import default_config as _defaults
from xingtian_amd.model.muzero.muzero_model import MuzeroModel, mlp_spec
from xingtian_amd.register import Registers


@Registers.model
class MuzeroMlp(MuzeroModel):
    def make_spec(self, model_info):
        cfg = model_info.get("model_config") or {}
        return mlp_spec(self.state_dim, self.action_dim, int(cfg.get("HIDDEN1_UNITS", _defaults.HIDDEN1_UNITS)),
                        int(cfg.get("HIDDEN2_UNITS", _defaults.HIDDEN2_UNITS)), self.td_step,
                        (self.value_min, self.value_max), (self.reward_min, self.reward_max), self.obs_type)
