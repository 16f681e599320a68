"""Module-level defaults of the DQN models (xt/model/dqn/default_config.py); YAML keys override them via import_config."""

HIDDEN_SIZE = 128
NUM_LAYERS = 1
LR = 0.0003
