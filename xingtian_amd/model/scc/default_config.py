"""Defaults of ``SCCModel``'s ``model_config`` (xt/model/scc/scc_tf.py:69-85 and examples/ma_cases/scc.yaml)."""

gamma = 0.99
c_lr = 0.0005
a_lr = 0.0005
mixer_grad_norm_clip = 10
actor_grad_norm_clip = 10
use_double_q = True
adam_beta1, adam_beta2, adam_epsilon = 0.9, 0.999, 1e-8      # tf.train.AdamOptimizer(c_lr)
rms_decay, rms_epsilon = 0.9, 1e-10                          # tf.train.RMSPropOptimizer(a_lr): momentum 0, not centred
# agents per unit type of the maps the reference knows; every other map is one group of all agents
agent_groups = {"2s3z": [2, 3], "3s5z": [3, 5], "3s5z_vs_3s6z": [3, 5], "1c3s5z": [1, 3, 5], "MMM2": [1, 2, 7]}
