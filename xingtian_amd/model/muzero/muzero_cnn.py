"""``MuzeroCnn`` (xt/model/muzero/muzero_cnn.py): the x / 255 conv trunk + Dense HIDDEN_OUT representation, hidden width
HIDDEN_OUT; ``obs_type`` uint8, float32 or int8 (uint8 frames read wrapped, as the reference's int8 placeholder does); see
``muzero_model``."""
from xingtian_amd.model.muzero import default_config as _defaults
from xingtian_amd.model.muzero.muzero_model import MuzeroModel, cnn_spec
from xingtian_amd.register import Registers


@Registers.model
class MuzeroCnn(MuzeroModel):
    def make_spec(self, model_info):
        cfg = model_info.get("model_config") or {}
        return cnn_spec(self.state_dim, self.action_dim, int(cfg.get("HIDDEN_OUT", _defaults.HIDDEN_OUT)), self.td_step,
                        (self.value_min, self.value_max), (self.reward_min, self.reward_max), self.obs_type)
