"""Counterparts of the reference's misc_scripts that drive the learner step by step (continual-learning accuracy matrix,
representation change); plots and result files stay with the caller.  CCA and CKA of the representations run on the GPU
(``rc_vision.run_rep_cca`` / ``rc_vision.run_rep_cka``).  ``cl_rl.run_cl_rl_exp`` is the continual-learning matrix of a policy on Particles2D
goals, adapted through ``learner.adapt(vpg_a2c_loss(...))``, ``single_ppo_update`` or ``trpo_update``."""
