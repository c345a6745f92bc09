"""MI355X-native batched SALP simulator (HIP/CDNA4 kernels behind a C ABI).

Public entry points (imported lazily so that the ABI description can be used
without torch or a GPU):

* :class:`grasp_lab_salp_amd.batched_env.BatchedSalpEnv` — n envs on one GPU,
  torch tensors in and out.
* :class:`grasp_lab_salp_amd.salp_robot_env.SalpRobotEnv`,
  :class:`grasp_lab_salp_amd.robot.Robot`, :class:`grasp_lab_salp_amd.robot.Nozzle`
  — drop-in replacements for the reference classes (src/salp_robot_env.py,
  src/robot.py).
* :class:`grasp_lab_salp_amd.vec_env.SalpVecEnv` — SB3 VecEnv-shaped adapter.
* :class:`grasp_lab_salp_amd.ppo.PPO`,
  :class:`grasp_lab_salp_amd.recurrent_ppo.RecurrentPPO`,
  :class:`grasp_lab_salp_amd.sac.SAC` — on-device learners (SAC is the one
  src/train_robot.py trains with).
* :mod:`grasp_lab_salp_amd.callbacks` — SB3-named training callbacks for SAC
  (metrics, evaluation, checkpoints); :mod:`grasp_lab_salp_amd.metrics` — the
  episode window and evaluation bookkeeping they keep on the device.
"""
__version__ = "0.1.0"
