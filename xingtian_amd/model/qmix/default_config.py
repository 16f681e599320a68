"""Defaults of ``QMixModel``'s ``model_config`` (xt/model/qmix/qmix_tf.py:49-67 and examples/ma_cases/qmix.yaml)."""

gamma = 0.99
lr = 0.0005
grad_norm_clip = 10
use_double_q = True
rms_decay = 0.95             # RMSPropOptimizer(lr, decay=0.95, epsilon=1.5e-7, centered=True)
rms_epsilon = 1.5e-7
