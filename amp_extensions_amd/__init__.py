"""amp_extensions_amd — MI355X-native learned-dynamics rollout path of amp_extensions.

The gym_simenv learned-dynamics step (4-model dense-MLP ensemble), the MILO RFF-MMD
cost and its MLP-feature variant with the ensemble-disagreement bonus, the AMP/GAIL least-squares discriminator
reward and the humanoid3d fall/horizon termination, as hand-written HIP kernels for
gfx950 behind a C ABI (include/amx_hip.h, libamx_hip.so) and the reference's Python
surfaces (SimEnv, sample_points, RBFLinearCost, MLPCost, GAILCost, DynamicsEnsemble), plus the
sampler's consumers: returns, MLP value baseline (prediction and the mini-batch Adam fit) and
GAE (mjrl process_samples, MLPBaseline), the NPG and PPO policy updates (mjrl npg_cg, ppo_clip)
and the behaviour-cloning warm start (mjrl BC), and the evaluation's DTW score of a rollout against
the reference motion (DeepMimicCore's time warper; TimeWarper, and evaluate.evaluate: the
submodule keeps the function's name, so it is imported from there).

The native library is loaded on first use; there is no CPU fallback.
"""
from .humanoid import TerminationConfig  # noqa: F401

__all__ = [
    "AmxContext", "DeviceEnsemble", "RffMap", "MlpMap", "RolloutEngine", "RBFLinearCost", "MLPCost", "GAILCost",
    "DevicePolicy",
    "TerminationConfig", "SimEnv", "BatchedSimEnv", "sample_points", "DeviceMLPBaseline", "process_samples",
    "DeviceNPG", "AgentReplayBuffer", "BC", "DeviceBC", "plan_bc_batches",
    "PPO", "DevicePPO", "NPG", "TimeWarper", "PlainDynamicsEnsemble", "dynamics_ensemble",
]


def __getattr__(name):
    if name in ("AmxContext", "DeviceEnsemble", "RffMap", "MlpMap"):
        from . import engine
        return getattr(engine, name)
    if name in ("RBFLinearCost", "MLPCost", "GAILCost"):
        from . import costs
        return getattr(costs, name)
    if name == "AgentReplayBuffer":
        from .datasets import AgentReplayBuffer
        return AgentReplayBuffer
    if name == "DevicePolicy":
        from .policy import DevicePolicy
        return DevicePolicy
    if name == "RolloutEngine":
        from .rollout import RolloutEngine
        return RolloutEngine
    if name in ("SimEnv", "BatchedSimEnv"):
        from . import sim_env
        return getattr(sim_env, name)
    if name in ("DeviceMLPBaseline", "process_samples"):
        from . import gae
        return getattr(gae, name)
    if name in ("DeviceNPG", "NPG"):
        from . import npg
        return getattr(npg, name)
    if name in ("BC", "DeviceBC", "plan_bc_batches"):
        from . import bc
        return getattr(bc, name)
    if name in ("PPO", "DevicePPO"):
        from . import ppo
        return getattr(ppo, name)
    if name in ("PlainDynamicsEnsemble", "dynamics_ensemble"):
        from . import ensemble
        return getattr(ensemble, name)
    if name == "TimeWarper":
        from .dtw import TimeWarper
        return TimeWarper
    if name == "sample_points":
        from .sampler import sample_points
        return sample_points
    raise AttributeError(name)
