"""Module-level defaults of the MuZero models (xt/model/muzero/default_config.py); ``model_config`` keys override them via
import_config.  ``max_value`` is carried as the reference carries it: nothing reads it."""

HIDDEN1_UNITS = 64
HIDDEN2_UNITS = 4
LR = 1e-3
td_step = 5
max_value = 500
HIDDEN_OUT = 256
