"""Module-level defaults of the DQN algorithm (xt/algorithm/dqn/default_config.py); YAML keys override them via
import_config.  TAU, LRC and UPDATE_FREQ are carried as the reference carries them: nothing in DQN reads them."""

TAU = 0.001
LRC = 0.001
BATCH_SIZE = 32
BUFFER_SIZE = 100000
TARGET_UPDATE_FREQ = 1000
GAMMA = 0.99
UPDATE_FREQ = 64
