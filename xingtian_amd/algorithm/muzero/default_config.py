"""Module-level defaults of the MuZero algorithm (xt/algorithm/muzero/default_config.py); YAML keys override them via
import_config."""

BATCH_SIZE = 1024
BUFFER_SIZE = 100000
GAMMA = 0.997
TD_STEP = 10
UNROLL_STEP = 5
