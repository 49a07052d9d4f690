"""Mirror of the reference's ``core_functions`` package for the vision MAML/ANIL hot path."""
from .vision import fast_adapt, accuracy, evaluate, meta_batch_adapt, meta_batch_adapt_steps, evaluate_steps, msl_weights
from .vision_models import OmniglotCNN, MiniImagenetCNN, ConvBase, ConvBlock
from .maml import MAML
from .inner_lr import InnerLR
from .step_offsets import StepOffsets
from .anil import meta_batch_adapt_anil, meta_batch_adapt_anil_steps
from .metric import meta_batch_adapt_metric, fast_adapt_metric, evaluate_nil
from .ridge import RidgeHead, meta_batch_adapt_ridge, fast_adapt_ridge, evaluate_ridge
from .logreg import LogRegHead, meta_batch_adapt_logreg, fast_adapt_logreg, evaluate_logreg
from .proto_anil import ProtoInit, meta_batch_adapt_proto_anil, fast_adapt_proto_anil, evaluate_proto_anil
from ..utils.data_pre import prepare_batch
from .policies import DiagNormalPolicy, DiagNormalPolicyANIL
from .rl import (fast_adapt_trpo, meta_optimize_trpo, meta_surrogate_loss, trpo_update, trpo_a2c_loss, fast_adapt_vpg, fast_adapt_ppo,
                 evaluate_vpg, evaluate_ppo, evaluate_trpo,
                 compute_advantages, set_device, LinearValue, Particles2DRunner, Particles2DEnv, EnvRunner, get_ep_successes,
                 rollout_tasks, fast_adapt_trpo_tasks, fast_adapt_vpg_tasks, fast_adapt_ppo_tasks, single_ppo_update, AdaptedTasks)
