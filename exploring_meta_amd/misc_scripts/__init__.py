"""Counterparts of the reference's misc_scripts that drive the learner step by step (continual-learning accuracy matrix,
representation change); plots and result files stay with the caller.  CCA and CKA of the representations run on the GPU
(``rc_vision.run_rep_cca`` / ``rc_vision.run_rep_cka``)."""
