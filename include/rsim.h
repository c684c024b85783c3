/*
 * rsim.h -- C-ABI of librsim_hip.so, the MI355X backend that replaces robosuite's MjSim hot path.
 *
 * Every entry point names the reference interface it stands in for (paths relative to the robosuite
 * checkout).  All functions return 0 on success, non-zero on error (message via rsim_last_error()).
 * Handles are opaque; the library owns all device memory; host buffers are owned by the caller.
 * No callbacks into the host language.  Thread-compatible per batch handle (one HIP stream per batch).
 */
#ifndef RSIM_H
#define RSIM_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rsim_model rsim_model;
typedef struct rsim_batch rsim_batch;

/* Built-in controller description: OSC_POSE arm + GRIP gripper.
 * Replaces controllers/parts/arm/osc.py:120-224 (constructor arguments) and
 * controllers/parts/gripper/simple_grip.py:62-107; index tables are what
 * robots/robot.py:300-333 (`setup_references`) resolves by name. */
/* arm part-controller types with an in-kernel implementation (names = the reference's `type` strings, controller_factory.py:93-147):
 *   OSC_POSE       arm/osc.py, control_dim 6            OSC_POSITION  arm/osc.py with use_ori=False, control_dim 3 (zero orientation delta, osc.py:255-263)
 *   JOINT_POSITION generic/joint_pos.py:200-266, control_dim ndof: goal = q + scaled delta, tau = M_arm (kp (goal - q) - kd qd) + qfrc_bias
 *   JOINT_TORQUE   generic/joint_tor.py:111-167, control_dim ndof: tau = clip(scaled action, torque_limits) + qfrc_bias
 *   JOINT_VELOCITY generic/joint_vel.py:129-209, control_dim ndof: PID on the joint-velocity error (kp per joint, ki = 0.005 kp, kd = 0.001 kp over a
 *                  5-tap mean of the error increments, integrator frozen while the part's torques saturate) + qfrc_bias, clipped to the actuator range.
 *                  The reference constructor raises in the surveyed snapshot (joint_vel.py:118 assigns to a read-only property); the law implemented
 *                  is that file's run_controller with the defect resolved as use_torque_compensation = True.
 * The action row of rsim_control_step is [control_dim arm entries, 1 gripper entry if ngrip > 0]. */
enum rsim_ctrl_type { RSIM_CTRL_OSC_POSE = 0, RSIM_CTRL_OSC_POSITION = 1, RSIM_CTRL_JOINT_POSITION = 2, RSIM_CTRL_JOINT_TORQUE = 3, RSIM_CTRL_JOINT_VELOCITY = 4 };
#define RSIM_JNT_MAX 16
typedef struct rsim_ctrl_desc {
  int32_t ndof;            /* controlled joints: <= 8 for the OSC types (one arm); <= 16 for the joint-space types, where the arms of a multi-arm
                            * robot are concatenated in `robot.arms` order (= the order CompositeController slices the action, composite_controller.py:97-103) */
  int32_t qpos_idx[RSIM_JNT_MAX];     /* Controller.qpos_index */
  int32_t dof_idx[RSIM_JNT_MAX];      /* Controller.qvel_index */
  int32_t act_idx[RSIM_JNT_MAX];      /* robot._ref_actuators_indexes_dict[arm] */
  int32_t eef_site;        /* site id of Controller.ref_name */
  int32_t base_site;       /* site id of f"{naming_prefix}{part_name}_center" (osc.py:453) */
  float kp[RSIM_JNT_MAX];  /* osc.py:176 (6 task-space gains) / joint_pos.py:150 (ndof joint gains) */
  float damping_ratio;     /* kd = 2 sqrt(kp) damping_ratio, osc.py:177, joint_pos.py:151 */
  float input_min[RSIM_JNT_MAX], input_max[RSIM_JNT_MAX], output_min[RSIM_JNT_MAX], output_max[RSIM_JNT_MAX]; /* controller.py:149-168, first control_dim entries used */
  int32_t uncouple_pos_ori; /* osc.py:476-482 */
  float nullspace_kp;       /* control_utils.py:7 (default 10) */
  int32_t ngrip;            /* gripper actuators (<= 4), 0 = no gripper */
  int32_t grip_act[4];
  float grip_sign[4];       /* PandaGripper.format_action direction, models/grippers/panda_gripper.py:55-57 */
  float grip_speed;         /* panda_gripper.py:61 */
  int32_t type;             /* enum rsim_ctrl_type: which arm part controller of controller_factory.py:73-159 */
  float torque_min[RSIM_JNT_MAX], torque_max[RSIM_JNT_MAX]; /* RSIM_CTRL_JOINT_TORQUE: torque_limits (joint_tor.py:95-96; default = actuator ctrlrange);
                                                             * RSIM_CTRL_JOINT_VELOCITY: velocity_limits (joint_vel.py:113, 147-148; all zero = none) */
  int32_t impedance_mode;             /* 0 "fixed", 1 "variable": action = [damping_ratio x n, kp x n, goal update], 2 "variable_kp": [kp x n, goal update]
                                       * (osc.py:243-253 with n = 6, joint_pos.py:204-214 with n = ndof): kp = clip(kp, kp_limits),
                                       * kd = 2 sqrt(kp) clip(damping_ratio, damping_ratio_limits) (1 in mode 2), applied from this control step on */
  float kp_min[RSIM_JNT_MAX], kp_max[RSIM_JNT_MAX], damping_min[RSIM_JNT_MAX], damping_max[RSIM_JNT_MAX];
  int32_t interp_steps;               /* 0: no interpolator; > 0: LinearInterpolator.total_steps = ceil(ramp_ratio * controller_freq / policy_freq)
                                       * (utils/traj_utils.py:25-155, controller_factory.py:87-94).  Restated as it is: set_goal moves start := previous
                                       * GOAL (not the value reached) and step := 0; each run_controller uses start + (goal - start) / (total - step)
                                       * and advances step up to total - 1.  Joint-space types interpolate their goal vector; OSC_POSITION its goal_pos,
                                       * which the reference then uses as a WORLD position although it holds base-frame coordinates (osc.py:418-423).
                                       * OSC_POSE adds the orientation interpolator (controller_factory.py:102-106, osc.py:277-283, 433-437): set_goal
                                       * stores orientation_error(goal_ori, current eef ori) as the new goal VECTOR, run_controller takes
                                       * mat2euler(slerp(quat(euler start), quat(euler goal), (step + 1) / total)) as its orientation error
                                       * (traj_utils.py:129-146: the error vectors are handled as Euler angles). */
  int32_t part_of[RSIM_JNT_MAX];      /* joint-space types: which part controller (arm) owns joint i; JOINT_POSITION multiplies by that part's own
                                       * mass-matrix block only (joint_pos.py:256-259 uses Controller.mass_matrix of the part) */
  int32_t narm;                       /* OSC types: number of arm parts, 1 (0 is read as 1) or 2.  Two = one OperationalSpaceController object per arm, as
                                       * CompositeController builds them for a bimanual robot (composite_controller.py:70-121, default_baxter.json): each
                                       * arm runs its own torque law on its own mass-matrix block (Controller.mass_matrix of the part, controller.py:226-233),
                                       * around its own "<arm>_center" origin site.  The second arm's joints / gains / action limits sit at entries
                                       * [8, 8 + ndof2) of qpos_idx / dof_idx / act_idx and [8, 14) of kp / input_* / output_*; its slice of the action row follows
                                       * the first arm's control_dim entries (and that arm's gripper entry).  damping_ratio, uncouple_pos_ori and nullspace_kp
                                       * are shared.  Not combined with impedance modes or interpolators. */
  int32_t ndof2, eef_site2, base_site2;
} rsim_ctrl_desc;

/* On-device observation / reward epilogue of the fused control step.
 * Observation record = robosuite's per-key observables concatenated in `_get_observations` order (environments/base.py:429-465),
 * one float per entry of `obs_prog`; every entry is (kind, a, b):
 *   RSIM_OBS_QPOS/COS/SIN/QVEL/QACC: joint quantity at address a          (robots/robot.py:334-394)
 *   RSIM_OBS_SITE_POS: site a, component b                                 (robot.py:412-414 eef_pos)
 *   RSIM_OBS_BODY_QUAT / RSIM_OBS_SITE_QUAT: body / site a, xyzw comp b    (robot.py:416-462; T.convert_quat / T.mat2quat)
 *   RSIM_OBS_BODY_POS: body a, component b                                 (lift.py:371-373 cube_pos)
 *   RSIM_OBS_BODY_MINUS_SITE: body a minus site (b >> 2), component b & 3  (manipulation_env.py:218-242 gripper_to_cube_pos)
 *   RSIM_OBS_BODY_MINUS_BODY: body a minus body (b >> 2), component b & 3  (stack.py:432-438 cubeA_to_cubeB = cubeB_pos - cubeA_pos)
 *   RSIM_OBS_PEG_COS / _T / _D: `angle`, `t`, `d` of TwoArmPegInHole._compute_orientation (two_arm_peg_in_hole.py:462-486, 523-560) between
 *                             object_body (peg) and object2_body (hole)
 *   RSIM_OBS_REL_POS / REL_QUAT: `{obj}_to_{arm}eef_pos / _quat` of PickPlace (manipulation_env.py:244-329, pick_place.py:639-668): pose of object a
 *                             (index into objects[]) in the gripper frame {eef_pos = grip_site, eef_quat = eef_body}, component b.  As in the
 *                             reference, the OBJECT pose is the one sampled at the previous control step (the relative sensors run before the
 *                             object's own pos / quat sensors and read them from the observation cache) while the gripper pose is current; after
 *                             rsim_observe (reset) they are zero.  pos_slot[a] = offset of `{obj}_pos` (3 floats, followed by `{obj}_quat` xyzw)
 *                             in the observation record.
 *   RSIM_OBS_TASK_OBJECT: the `obj_id` observable of PickPlace single-object mode 1 (pick_place.py:626-635): RSIM_TASK_OBJECT of the env as a float;
 *                             in that mode a = -1 in REL_POS / REL_QUAT / BODY_POS / BODY_QUAT means "the env's current object" (its root body).
 * Sampling instants follow the reference exactly: after `reset()` every Observable samples on the LAST substep of a control step,
 * i.e. positions/orientations come from that substep's step1 kinematics, qpos/qvel from after its step2 (utils/observables.py:214-259).
 * task 1: reward = Lift.reward (environments/manipulation/lift.py:224-273), success = Lift._check_success (lift.py:433-444),
 * grasp = ManipulationEnv._check_grasp on the contact list (manipulation_env.py:331-376).
 * task 2: reward = Stack.reward / staged_rewards (environments/manipulation/stack.py:224-312) with object = cubeA, object2 = cubeB
 * (reach + grasp, lift + align, stack = lifted, released and cubeA touching cubeB via check_contact, utils/sim_utils.py:8-40),
 * success = Stack._check_success (stack.py:476-484: r_stack > 0); scaled by reward_scale / 2.0.
 * task 3: reward = TwoArmPegInHole.reward (two_arm_peg_in_hole.py:240-290) with object = peg, object2 = hole: success (d < 0.06, -0.12 <= t <= 0.14,
 * cos > 0.95; :513-521) + reaching + perpendicular / parallel distance + alignment terms, scaled by reward_scale / 5.0.
 * task 4: reward = PickPlace.reward / staged_rewards / _check_success (pick_place.py:274-429, 737-762) over nobj objects (all-objects mode): objects
 * in their bins + max(reach, grasp, lift, hover) over the others, scaled by reward_scale / 4.0; success = every object in its bin
 * (single_object_mode != 0: scaled by reward_scale, success = any object in its bin). */
enum { RSIM_OBS_QPOS = 0, RSIM_OBS_COS, RSIM_OBS_SIN, RSIM_OBS_QVEL, RSIM_OBS_QACC, RSIM_OBS_SITE_POS, RSIM_OBS_BODY_QUAT, RSIM_OBS_SITE_QUAT,
       RSIM_OBS_BODY_POS, RSIM_OBS_BODY_MINUS_SITE, RSIM_OBS_BODY_MINUS_BODY, RSIM_OBS_PEG_COS, RSIM_OBS_PEG_T, RSIM_OBS_PEG_D,
       RSIM_OBS_REL_POS, RSIM_OBS_REL_QUAT, RSIM_OBS_TASK_OBJECT };
#define RSIM_OBS_MAX 128
typedef struct rsim_task_desc {
  int32_t nobs;                       /* floats in the observation record (<= RSIM_OBS_MAX) */
  int32_t obs_prog[RSIM_OBS_MAX * 3]; /* (kind, a, b) per output float */
  int32_t task;                       /* 0 = none, 1 = Lift, 2 = Stack, 3 = TwoArmPegInHole, 4 = PickPlace */
  int32_t object_body;                /* cube root body */
  int32_t grip_site;                  /* gripper.important_sites["grip_site"] */
  float table_height;                 /* model.mujoco_arena.table_offset[2] */
  float lift_margin;                  /* 0.04 */
  float reward_scale;                 /* reward_scale (1.0), applied as reward_scale / 2.25 */
  int32_t reward_shaping;
  uint64_t left_pad_geoms, right_pad_geoms, object_geoms; /* bit g set: colliding-geom index g belongs to the group (_check_grasp) */
  int32_t object2_body;               /* Stack: cubeB root body */
  uint64_t object2_geoms;             /* Stack: cubeB contact geoms */
  /* PickPlace (task 4) */
  int32_t nobj;                       /* objects (<= 4), bin i is the target of object i */
  int32_t obj_body[4];                /* object root bodies */
  uint64_t obj_geoms[4];              /* contact geoms per object (colliding-geom bit masks) */
  int32_t pos_slot[4];                /* offset of `{obj}_pos` in the observation record (see RSIM_OBS_REL_POS) */
  int32_t eef_body;                   /* body whose quaternion is `{arm}eef_quat` */
  float bin2_pos[3], bin_size[2];     /* pick_place.py:188-199 */
  float bin_target[8];                /* target_bin_placements[i][0..1] (pick_place.py:570-583) */
  int32_t single_object_mode;         /* PickPlace: 0 = all objects; 1 = one object, drawn anew at every reset (PickPlaceSingle, pick_place.py:717-722, 800-807):
                                       * the env's current object id lives in RSIM_TASK_OBJECT -- set by the host's reset, and by the on-device episode reset
                                       * from the reset-bank column whose patch index is RSIM_PATCH_TASK_OBJECT -- observation entries with a = -1
                                       * (RSIM_OBS_REL_POS / REL_QUAT: object; RSIM_OBS_BODY_POS / BODY_QUAT: the object's root body) refer to it and
                                       * RSIM_OBS_TASK_OBJECT is the `obj_id` observable (:626-635); all pos_slot entries name the one `{obj}_pos` slot;
                                       * 2 = one fixed object (PickPlaceMilk / Bread / Cereal / Can, pick_place.py:800-847): the
                                       * reward is not divided by 4 (:308-310) and success = any object in its bin (:757-759).  The other objects stay in the
                                       * model -- the host's reset moves them to (10, 10, 10) (base.py:591-602) -- and in every sum of the reward, as in the reference */
} rsim_task_desc;

/* state / derived arrays addressable through rsim_get_array / rsim_set_array / rsim_device_ptr.
 * The derived arrays RSIM_XPOS .. RSIM_NITER and RSIM_SENSORDATA are written by rsim_forward / rsim_step1 / rsim_step2 / rsim_step / rsim_run_controller /
 * rsim_step2_last / rsim_observe; the fused rsim_control_step does not produce them.  Reading one of them (rsim_get_array, rsim_device_ptr, rsim_jac_*)
 * after a fused control step first runs rsim_forward on the current state -- the sim.forward() robosuite itself issues before it reads derived
 * quantities (base.py:298-303) -- so they are never the leftovers of an earlier launch. */
enum rsim_field {
  RSIM_QPOS = 0,       /* [B,nq]  sim.data.qpos   (binding_utils.py MjData.qpos)            */
  RSIM_QVEL,           /* [B,nv]  sim.data.qvel                                              */
  RSIM_QACC_WARMSTART, /* [B,nv]                                                            */
  RSIM_CTRL,           /* [B,nu]  sim.data.ctrl   (fixed_base_robot.py:153)                 */
  RSIM_TIME,           /* [B]     sim.data.time                                              */
  RSIM_CSTATE,         /* [B,cs]  controller state, cs = rsim_model_int(m, "cstate_size"): OSC types (32) goal_pos3 goal_ori9 q0[8] grip[4] tau[8];
                        *          joint-space types (64) goal[16] - grip[4] at 20 - tau[16] at 32; JOINT_VELOCITY (192) adds last_err[16] at 48,
                        *          summed_err[16] at 64, derr ring[5][16] at 80, ring ptr / size at 160 / 161, saturated[part] at 164;
                        *          variable-impedance modes (128): current kp[16] at 96, kd[16] at 112;
                        *          interpolator (200): start[16] at 180, step at 196; OSC_POSE orientation interpolator start[3] at 184, goal[3] at 188 */
  RSIM_XPOS,           /* [B,nbody,3]  sim.data.xpos      (derived, valid after forward/step1) */
  RSIM_XQUAT,          /* [B,nbody,4]  sim.data.xquat                                        */
  RSIM_QM,             /* [B,nv,nv]    dense mass matrix (mj_fullM, controller.py:226-227)  */
  RSIM_QFRC_BIAS,      /* [B,nv]       sim.data.qfrc_bias (controller.py:303-311)           */
  RSIM_QFRC_PASSIVE,   /* [B,nv] */
  RSIM_QFRC_ACTUATOR,  /* [B,nv] */
  RSIM_QFRC_CONSTRAINT,/* [B,nv] */
  RSIM_QACC,           /* [B,nv]       sim.data.qacc                                         */
  RSIM_CDOF,           /* [B,nv,6]     motion axes about the tree COM (for Jacobians)       */
  RSIM_ROOTCOM,        /* [B,nbody,3]  subtree COM per tree root                            */
  RSIM_CONTACT,        /* [B,maxcon,24] dist pos3 frame9 geom1 geom2 dim efc_adr fn friction5 */
  RSIM_EFC_FORCE,      /* [B,maxefc] */
  RSIM_NCON,           /* [B] int32    sim.data.ncon                                         */
  RSIM_NEFC,           /* [B] int32 */
  RSIM_NITER,          /* [B] int32    solver iterations of the last substep                 */
  RSIM_OBS,            /* [B,nobs]     observation record of the last control step (float32) */
  RSIM_REWARD,         /* [B]          reward of the last control step                       */
  RSIM_SUCCESS,        /* [B] int32    _check_success() after the last control step          */
  RSIM_DONE,           /* [B] int32    timestep >= horizon after the last control step (base.py:532-548) */
  RSIM_EP_STEP,        /* [B] int32    MujocoEnv.timestep of the running episode            */
  RSIM_EP_INDEX,       /* [B] int32    number of the running episode (0, 1, 2, ...; its reset came from bank slot number % n_episodes) */
  RSIM_DIVERGED,       /* [B] int32    how often the env hit MuJoCo's bad-state guard: after a substep that leaves a non-finite or > 1e10 qpos / qvel
                        *               entry the env is put back to qpos0 with zero velocity, control and time, as mj_checkPos / mj_checkVel +
                        *               mj_resetData do [3P]; robosuite never reads the corresponding mjData warning, this counter makes it visible */
  RSIM_OVERFLOW,       /* [B] int32    contacts + constraint rows the env had to DROP since the batch was created because a substep found more than the
                        *               compiled capacity (rsim_batch_limits: 16 contacts / 64 rows in the Lift configuration, 128 rows in the largest).
                        *               MuJoCo's nconmax = 5000 (models/assets/base.xml:5) never truncates; a non-zero count marks results that can differ
                        *               from the reference for that reason */
  RSIM_BANK_STALE,     /* [B] int32    on-device resets that found a reset-bank slot the host had not refilled in time (the stale entry was used):
                        *               0 as long as rsim_refill_reset_bank keeps up, i.e. no reset is ever replayed */
  RSIM_TERMINAL_OBS,   /* [B,nobs]     observation record of the control step that ENDED an env's episode (valid where RSIM_DONE was reported); with a reset
                        *               bank installed RSIM_OBS of such an env already holds the observation MujocoEnv.reset() returns for its next
                        *               episode (gym auto-reset convention), the reward / success flags stay those of the terminal step */
  RSIM_SENSORDATA,     /* [B,nsensordata] mjData.sensordata (binding_utils.py:935-938; Robot.get_sensor_measurement, robots/robot.py:739-751), MuJoCo's semantics
                        *               [3P, docs "XML reference: sensor"].  <force> / <torque> at a site (the grippers' ft_frame) as mj_sensorAcc evaluates them --
                        *               the wrench the site body's parent transmits to it, from the solved accelerations and contact forces, in the site frame.
                        *               Carried besides them: jointpos, jointvel (hinge / slide), tendonpos, tendonvel (fixed tendons), framepos, framequat,
                        *               framelinvel, frameangvel (objtype site | xbody | body), velocimeter, gyro, accelerometer (at a site), touch (sphere,
                        *               ellipsoid or box site), actuatorfrc, and rangefinder (position stage: rsim_ray from the site along its +Z, the site's body
                        *               excluded, all groups, static geoms included; -1 when nothing is hit).  Written by rsim_forward / rsim_step2 / rsim_step / rsim_step2_last / rsim_observe:
                        *               the values of the last substep, before its integration; rsim_step1 / rsim_run_controller write the position- and
                        *               velocity-stage entries only and leave the acceleration-stage ones (force, torque, accelerometer, touch, actuatorfrc) as
                        *               they are, as mj_step1 does.  A sensor that is not carried -- another type, reftype / refname, objtype geom | camera, a
                        *               capsule or cylinder touch site, jointpos on a ball or free joint, a non-zero cutoff -- compiles and reads zero:
                        *               rsim_model_int("nsensor_zero") counts them, rsim_sensor_slice names them.  noise is ignored, as MuJoCo's simulation
                        *               ignores it.  rsim_model_int("nsensordata") gives the row length */
  RSIM_TASK_OBJECT,    /* [B] int32    PickPlace single-object mode 1: index of the object this env's current episode uses (see rsim_task_desc.single_object_mode) */
  RSIM_CAP_NEED,       /* [B,2] int32  largest number of contacts / constraint rows any substep of the env has asked for since the batch was created (what
                        *               RSIM_OVERFLOW's drops are measured against: a value above rsim_batch_limits means that substep was truncated);
                        *               sizes the compiled capacities against a workload (bench.py reports the maxima) */
  RSIM_QFRC_APPLIED,   /* [B,nv]       mjData.qfrc_applied: user-specified generalised forces, added to the smooth forces by rsim_forward / rsim_step1 / rsim_step2 /
                        *               rsim_step (the B = 1 compatibility entries: models/grippers/gripper_tester.py:197-202 writes its gravity compensation
                        *               there), and by rsim_control_step once rsim_set_applied_forces(b, 1) enabled it; zeroed by rsim_reset and, where it is
                        *               read, by the on-device episode restart.  By default the fused rsim_control_step does not read it -- nothing on robosuite's
                        *               env.step path writes qfrc_applied */
  RSIM_POLISH,         /* [B] int32    wide configurations, debug entries: how the fp64 polish behind the Newton iteration of the last substep ended (no MuJoCo counterpart;
                        *               solve_newton in csrc/rsim_step.hip): 10000 x passes + 100000 x floor(-log10 of the scaled fp64 gradient at the accepted point)
                        *               + 10^7 x exit (1 gradient below tolerance, 2 improvement below tolerance, 3 pass budget,
                        *               5 direction was no descent direction, 6 a step raised the objective; 0 not run) */
  RSIM_XFRC_APPLIED,   /* [B,nbody,6]  mjData.xfrc_applied: a Cartesian wrench per body -- force (3) then torque (3), world coordinates, applied at the body's COM
                        *               (xipos).  Added as J^T wrench to the smooth forces (mj_xfrcAccumulate) and to the body's cfrc_ext for the <force> / <torque>
                        *               sensors (mj_rnePostConstraint) wherever RSIM_QFRC_APPLIED is honoured, under the same switch; zeroed like it */ RSIM_END_REASON,
                       /* RSIM_END_REASON (the last field, = RSIM_XFRC_APPLIED + 1: appended, no existing value moves; on RSIM_XFRC_APPLIED's line because
                        *               tests/test_applied_forces_host.py pins that entry as the last one that starts a line) [B] int32: why the launch that reported RSIM_DONE ended the env's
                        *               episode -- 0 running, 1 horizon, 2 success, 3 bad-state guard, 4 requested.  Maintained by every control step while a rule of
                        *               rsim_set_early_end is armed and written (4) by rsim_end_episodes; with no rule armed the control step does not maintain it
                        *               (RSIM_DONE alone says "horizon") and it reads 0 after rsim_set_early_end(b, 0, ..) / rsim_reset */
  RSIM_FIELD_COUNT
};
#define RSIM_PATCH_TASK_OBJECT (-1)   /* rsim_set_reset_bank patch index: this column of a reset row is the episode's RSIM_TASK_OBJECT, not a float-table entry */

const char* rsim_last_error(void);

/* Ingests a compiled model blob ("RSIMMDL1": magic, entry table {name[32], dtype, count, offset}, 8-byte aligned payloads; written by rsim_mjcf_to_blob
 * below and by robosuite_amd.mjcf.to_blob).  Host only, no GPU. */
int rsim_model_create(const void* blob, size_t len, rsim_model** out);
/* mujoco.MjModel.from_xml_string itself (binding_utils.py:1077-1080; MujocoXML.get_model, models/base.py:125-147; the per-reset rebuild of
 * environments/base.py:262-269) for a host WITHOUT Python: the MJCF string robosuite assembles goes in, a model handle comes out.  The compiler is
 * robosuite_amd/csrc/rsim_mjcf.cpp (defaults classes, bodies / joints / geoms / sites, mesh loading + convex hulls + mesh inertia, inertia from geoms,
 * actuators, fixed tendons + tendon equalities, the collision pair list, names, the constants at qpos0: subtree masses and inverse weights); the Python
 * compiler robosuite_amd/mjcf.py is kept as its checker (tests/test_mjcf_cpp.py).  asset_dir (NULL = none) is what relative mesh file names are resolved
 * against, after <compiler meshdir>; robosuite writes absolute paths.  Malformed or unsupported MJCF fails with the reason in rsim_last_error(), as
 * MuJoCo's compiler raises.  Host only, no GPU.
 * rsim_mjcf_to_blob is the same compile stopping at the blob (what rsim_model_create ingests, what robosuite_amd.mjcf.to_blob writes): *blob is
 * malloc'ed and released with rsim_blob_free -- for binders that cache compiled models or ship them to other ranks. */
int rsim_model_compile(const char* xml, size_t len, const char* asset_dir, rsim_model** out);
int rsim_mjcf_to_blob(const char* xml, size_t len, const char* asset_dir, void** blob, size_t* blob_len);
void rsim_blob_free(void* blob);
void rsim_model_free(rsim_model* m);
/* scalar / size query by blob field name ("nq", "nv", ...); returns -1 if unknown.  Beyond the blob's fields: "nsensordata", and "nsensor_zero" = the
 * number of sensors that read zero because their type, object or an option of theirs is not carried (RSIM_SENSORDATA) */
int rsim_model_int(const rsim_model* m, const char* name);
/* Where sensor `sensor_id` (rsim_name2id(m, "sensor", ..)) sits in a row of RSIM_SENSORDATA: first entry, number of entries, and whether it is computed
 * (1) or reads zero (0).  Any of the three pointers may be NULL.  Non-zero return: bad id. */
int rsim_sensor_slice(const rsim_model* m, int sensor_id, int* adr, int* dim, int* carried);
/* Which compiled kernel configuration serves this model: 0 = 32 bodies x 16 dofs (Lift/Panda), 1 = 32 x 32 (Stack/Panda), 2 = 64 x 16 (Baxter);
 * 3 = 64 x 64 with tendon rows (PickPlace/IIWA+Robotiq140); -1 = none (rsim_batch_create would refuse it).  limits, if not NULL, receives 10 ints: {nbody, njnt, nv, ncgeom, nsite, ncon, nefc, npair, articulated trees} maxima
 * and a flag word: bit 0 = the configuration carries tendon / equality rows (the 32 x 16 one does not: such models go to the next larger one), bit 1 = two-arm
 * controller masks, bits 2 / 3 / 4 = the build keeps its constraint Jacobian / mass matrix / contact block in a per-env buffer in global memory instead of LDS
 * (an occupancy choice of the build, sized by rsim_batch_create; nothing a caller has to act on), bit 6 = the configuration carries ball joints (the 32 x 32 one:
 * a model with a ball joint that no such configuration holds is refused; limited ball joints are refused everywhere). */
int rsim_model_config(const rsim_model* m, int* limits);
/* mj_name2id / mj_id2name as robosuite's MjModel wrapper uses them (binding_utils.py:296-360: body_name2id, joint_name2id, geom_name2id, site_name2id,
 * actuator_name2id, camera_name2id, sensor_name2id, ... and the id2name inverses).  kind = "body" | "joint" | "geom" | "site" | "actuator" | "camera" | "light" |
 * "sensor" | "tendon" | "equality" | "mesh"; the names ride in the model blob (entries "names:<kind>").  rsim_name2id: id, or -1 if there is no such name;
 * rsim_id2name: the name (owned by the model, valid until rsim_model_free), or NULL for an unnamed object / a bad id. */
int rsim_name2id(const rsim_model* m, const char* kind, const char* name);
const char* rsim_id2name(const rsim_model* m, const char* kind, int id);
/* controller_factory (controllers/parts/controller_factory.py:73-159) for the built-in arm part (rsim_ctrl_type) + GRIP pair */
int rsim_model_set_controller(rsim_model* m, const rsim_ctrl_desc* desc);
/* observation / reward epilogue of rsim_control_step (must be set before rsim_batch_create) */
int rsim_model_set_task(rsim_model* m, const rsim_task_desc* desc);
/* colliding-geom index (bit position in rsim_task_desc geom masks) of a model geom id, -1 if the geom never collides */
int rsim_model_cgeom(const rsim_model* m, int geom_id);

/* mujoco.MjData(model) x B (binding_utils.py:586-590): allocates B environments on `device`.
 * per_env_params != 0 gives every env its own copy of the float model constants (domain randomisation,
 * per-episode object sizes); 0 shares one copy. */
int rsim_batch_create(rsim_model* m, int B, int device, int per_env_params, rsim_batch** out);
void rsim_batch_free(rsim_batch* b);
int rsim_batch_size(const rsim_batch* b);
int rsim_batch_limits(const rsim_batch* b, int* maxcon, int* maxefc);

/* mj_resetData (binding_utils.py:1091): qpos = qpos0, qvel = 0, ctrl = 0, time = 0 for envs with mask[i] != 0 (NULL = all) */
int rsim_reset(rsim_batch* b, const uint8_t* host_mask);
/* mj_forward / mj_step1 / mj_step2 / mj_step (binding_utils.py:1095-1107) on every env */
int rsim_forward(rsim_batch* b);
int rsim_step1(rsim_batch* b);
int rsim_step2(rsim_batch* b);
int rsim_step(rsim_batch* b);
/* Fused fast path = MujocoEnv.step's substep loop (environments/base.py:494-504) with the built-in controllers:
 * n_sub x { step1; control(action, policy_step = first); step2 } in ONE launch.  `actions_dev` is a DEVICE pointer
 * to [B, action_dim] float32 (action_dim = control_dim(type) + (ngrip>0); rsim_model_int(m, "action_dim")). */
int rsim_control_step(rsim_batch* b, const float* actions_dev, int n_sub);
/* CompositeController.run_controller() alone (composite_controller.py:109-116 -> osc.py:403-495, joint_pos.py:238-266, joint_vel.py:129-209,
 * simple_grip.py:150-186; the clip into ctrl: fixed_base_robot.py:143-153): mj_step1-equivalent position / velocity stage on the current state, then ONE
 * evaluation of the part controllers from RSIM_CSTATE as it stands (goals, initial joints, gripper action, PID state) -- no set_goal, no actuation, no
 * integration.  Results: RSIM_CTRL and the torque slots of RSIM_CSTATE (un-clipped tau, layout at enum rsim_field). */
int rsim_run_controller(rsim_batch* b);
/* The last rsim_step2 of a control step driven from the host side -- user part controllers evaluated on [B, ...] device tensors between rsim_step1 and
 * rsim_step2 of the whole batch (robosuite_amd/controllers.py, the batched form of the Controller plugin API, controllers/parts/controller.py:35-44,
 * 140-147): the substep's actuation / solve / integration, then what MujocoEnv.step does after its loop (base.py:508-548: timestep, reward, done) and
 * the observation record, with the on-device episode restart of rsim_control_step.  RSIM_DONE tells the caller which envs restarted. */
int rsim_step2_last(rsim_batch* b);
/* Robot.reset's controller re-creation (robots/robot.py:271 -> controller.py:125-131, osc.py:520-532):
 * forward kinematics, initial_joint := q, goal := current eef pose, gripper action := 0 */
int rsim_ctrl_reset(rsim_batch* b, const uint8_t* host_mask);
int rsim_sync(rsim_batch* b);
/* forward() + observation/reward epilogue without advancing time: the observation MujocoEnv.reset returns (base.py:298-347) */
int rsim_observe(rsim_batch* b);

/* Episode bookkeeping of MujocoEnv.step (base.py:508, 532-548): every rsim_control_step increments the per-env timestep and sets
 * RSIM_DONE when it reaches `horizon` (0 = never).  With a reset bank installed, a finished env is re-initialised ON THE DEVICE at the
 * end of that same launch: qpos := bank entry, qvel/ctrl/warm start/time := 0, the listed float-table entries (per-episode model edits
 * such as the Lift cube size, lift.py:311-318) are patched, and the controller is re-created at the start of the next launch
 * (robots/robot.py:271).  The same call then produces the observation MujocoEnv.reset() returns (forward + observables on the reset state)
 * in RSIM_OBS and keeps the finished episode's last record in RSIM_TERMINAL_OBS.
 * The bank is a RING of `n_episodes` (>= 2) slots per env: episode k of an env is read from slot k % n_episodes (RSIM_EP_INDEX counts
 * episodes for ever).  rsim_set_reset_bank fills slots with episodes 0 .. n_episodes-1 (drawn by the host in the reference's RNG order);
 * rsim_refill_reset_bank overwrites consumed slots with later episodes, so that every reset of every env is a fresh draw, as the
 * reference's hard reset is (base.py:277-347).  A reset that finds a slot not holding its episode is counted in RSIM_BANK_STALE.
 * bank: HOST float32 [B, n_episodes, nq + n_patch]; patch_idx: HOST int32 [n_patch] offsets into the env's float table
 * (rsim_param_offset).  Requires per_env_params when n_patch > 0.
 * rsim_refill_reset_bank: rows[i] (HOST float32 [n, nq + n_patch]) = reset `episode[i]` of env `env[i]`. */
int rsim_set_episode(rsim_batch* b, int horizon);
int rsim_set_reset_bank(rsim_batch* b, int n_episodes, int n_patch, const int32_t* patch_idx, const float* bank);
int rsim_refill_reset_bank(rsim_batch* b, int n, const int32_t* env, const int32_t* episode, const float* rows);
/* The same upkeep without ever stalling the control steps (the reference has no counterpart: its reset is a blocking recompile, base.py:277-347).
 * All three run on a side stream of the batch and neither wait for the control steps in flight nor make them wait; they may be called from a second
 * host thread while the first one keeps stepping (one upkeep thread per batch).
 *   rsim_bank_poll_begin          starts an asynchronous copy of RSIM_EP_INDEX into pinned host memory (at most one in flight);
 *   rsim_bank_poll                1 + the counters in ep_index[B] once that copy has landed, 0 while it is in flight (wait != 0: block), -1 on error.
 *                                 The counters only grow, so a copy taken beside running control steps is at worst slightly old;
 *   rsim_refill_reset_bank_async  like rsim_refill_reset_bank, through pinned staging, returns without waiting.  Only slots whose episode the env
 *                                 has already STARTED (episode <= polled counter) may be overwritten; the slot's tag is published after its row;
 *   rsim_bank_flush               returns when every refill issued so far is in the ring (tests, shutdown). */
int rsim_bank_poll_begin(rsim_batch* b);
int rsim_bank_poll(rsim_batch* b, int32_t* ep_index, int wait);
int rsim_refill_reset_bank_async(rsim_batch* b, int n, const int32_t* env, const int32_t* episode, const float* rows);
int rsim_bank_flush(rsim_batch* b);
/* offset of element `elem` of model float array `field` ("geom_size", "body_mass", ...) inside an env's float table, -1 if unknown */
int rsim_param_offset(const rsim_batch* b, const char* field, int elem);

/* Dispatch order of rsim_control_step (no reference counterpart; results do not depend on it).  longest_first != 0 (default): the envs that took
 * longest in the previous control step (contact-rich envs stay so for many steps) are handed to the first workgroups, which shortens the
 * tail of a launch; 0: env i = workgroup i. */
int rsim_set_schedule(rsim_batch* b, int longest_first);
/* External forces in the fused control step (off by default: no control-step kernel reads RSIM_QFRC_APPLIED / RSIM_XFRC_APPLIED and every result is what it
 * is without them).  enable = 1: every substep of rsim_control_step adds qfrc_applied + J^T xfrc_applied to the smooth forces, as mj_fwdAcceleration does.
 * The debug entries (rsim_forward, rsim_step*, rsim_step2_last) honour both arrays either way.  Wherever the arrays are read -- the control step with the
 * switch on, rsim_step2_last always -- the on-device episode restart zeroes both arrays of an env in the launch that reports its RSIM_DONE (mj_resetData, as
 * rsim_reset does), so a wrench written after that applies to the new episode; with the switch off the control step leaves them as they are. */
int rsim_set_applied_forces(rsim_batch* b, int enable);
/* Ending episodes before the horizon (the reference has no counterpart: MujocoEnv.step ends an episode at the horizon only, base.py:532-548; success and
 * divergence checks live in wrappers and training loops around it).  OFF BY DEFAULT: an unarmed batch launches nothing extra and computes what it always did.
 * Both entries need a reset bank (rsim_set_reset_bank) and fail without one: an episode that ends restarts, in the same call, from the env's next pre-drawn
 * reset -- exactly what the horizon does (see above: ring slot, patches, RSIM_TERMINAL_OBS, reset observation in RSIM_OBS, RSIM_DONE = 1, fresh controller
 * at the next step); RSIM_REWARD / RSIM_SUCCESS keep the terminal step's values.
 *   rsim_set_early_end  rules: bit 0 = end on success (RSIM_SUCCESS != 0 once the episode step counter, counted like `horizon`, is >= min_steps; min_steps >= 1),
 *                       bit 1 = end when the bad-state guard fired during the step (RSIM_DIVERGED grew: the env restarts from a drawn reset instead of carrying
 *                       on from qpos0 inside the same episode); 0 disarms.  While armed, every rsim_control_step / rsim_step2_last is followed on its stream(s) by
 *                       one small kernel (k_end_episodes) that decides per env, first match: 1 the step itself ended the episode at the horizon (never restarted
 *                       twice), 2 success, 3 diverged -- and writes RSIM_END_REASON for every env.  Guard hits from before the call (or before rsim_reset) do not count.
 *   rsim_end_episodes   ends NOW the running episode of every env with mask_dev[env] != 0 (DEVICE uint8 [B]), outside a control step: restart from the ring +
 *                       reset observation, RSIM_DONE = 1 and RSIM_END_REASON = 4 for those envs, every other env untouched (their RSIM_DONE included).  The reset
 *                       observation is taken as rsim_observe takes it after a host reset, for the ended envs only: an env ended here is bit for bit the env a host
 *                       reset of its next episode builds.  Consumes a ring slot per ended env: refill before the ring runs dry (RSIM_BANK_STALE counts a miss). */
int rsim_set_early_end(rsim_batch* b, int rules, int min_steps);
int rsim_end_episodes(rsim_batch* b, const uint8_t* mask_dev);
/* Stream groups of rsim_control_step (no reference counterpart; results do not depend on it).  A control step lasts as long as its slowest env
 * (contact-rich envs take 3-4 x the median) and the envs are independent, so with groups = G > 1 the batch is stepped as G contiguous env
 * blocks, each on its own HIP stream: block g's step t + 1 starts as soon as ITS envs have finished step t, filling the CUs that the other
 * blocks' stragglers leave idle.  The caller's view is unchanged -- one call enqueues one step of all envs; rsim_sync() and every entry point
 * that reads or writes batch state first wait for all groups; the actions buffer of a step must stay untouched until then.  1 = one launch
 * on the batch's stream (default).  groups <= 32 and <= the batch size. */
int rsim_set_stream_groups(rsim_batch* b, int groups);
void* rsim_group_stream(rsim_batch* b, int group);   /* hipStream_t the control steps of env block `group` run on (for event timing) */

/* Per-phase cycle accounting of the fused kernel (no reference counterpart: the reference has no profiling).
 * enable != 0 (re)arms and zeroes the accumulators, 0 disarms; if `out` is non-NULL the current accumulators are copied out first:
 * cycles {load kin com crb broad narrow makec vel ctrl act solve euler store} then counts {substeps candidates contacts efc newton ls}. */
int rsim_profile(rsim_batch* b, int enable, unsigned long long* out, int n_out);
/* While profiling is armed every launch also logs, per env, {HW_ID, XCC_ID, start, end (s_memrealtime ticks, 100 MHz), #MPR runs, #support
 * evaluations, #Newton iterations, #broadphase candidates}: out = HOST u64 [B,8]. */
int rsim_wavelog(rsim_batch* b, unsigned long long* out);
/* restrict the phase accumulators to one env (-1 = all envs) */
int rsim_profile_env(rsim_batch* b, int env);
/* Capacity tier of every env for the NEXT control step, HOST int32 [B]: 0 = stepped by the batch's native kernel configuration, 1 = by the wider one (MuJoCo
 * never truncates contacts -- nconmax = 5000, models/assets/base.xml:5 -- so an env that outgrows the native contact / row capacity is stepped with more).
 * Synchronises the batch's stream.  No reference counterpart (diagnostics: which envs a lockstep launch waits for). */
int rsim_tier_snapshot(rsim_batch* b, int* host_tier);
/* Restart flag of every env, HOST int32 [B]: 1 = a control step (or rsim_end_episodes) re-initialised the env from its reset ring and the next rsim_control_step
 * starts it with fresh controller objects (robots/robot.py:271), then clears the flag.  Synchronises the batch's stream.  Diagnostics. */
int rsim_restart_flags(rsim_batch* b, int* host_flags);
/* The host-side settings that decide what a control step dispatches and how its solver stops -- compiled-in defaults and the RSIM_* environment overrides in
 * force -- as one string (valid until the next call).  Measurement files carry its sha next to the kernel's: evidence of other settings is not this build's. */
const char* rsim_tuning_defaults(void);
/* out2[0] = env-steps (env x control step) the wider capacity tier stepped since the batch was created, out2[1] = how many of them changed tier in mid-step
 * (carried on from the substep in which they outgrew the native capacity, or redone).  Synchronises the batch's stream.  bench.py reports both. */
int rsim_tier_stats(rsim_batch* b, unsigned long long* out2);
/* Configurations 0-2 compile the control step twice: a plain kernel, and a full one that also holds the profiler (rsim_profile), the MPR restart cone
 * (RSIM_MPR_CONE) and the applied forces (rsim_set_applied_forces) behind their run-time switches; a launch takes the full one while any of the three is in
 * use, or always when RSIM_FULL_STEP_KERNEL=1 was set when the batch was created.  Both compute the same bits.  out2[0] = launches of the plain kernel,
 * out2[1] = of the full one, since the batch was created (0, 0 for the other configurations).  No synchronisation.  Diagnostics. */
int rsim_step_kernel_launches(rsim_batch* b, unsigned long long* out2);
/* The narrow phase's warm-start records as the last launch left them: HOST float32 [B][npair][12] (npair = rsim_model_int "npair"; per pair: a direction or
 * depth, a flag -- 0 nothing known, 1 separating direction, 2 portal directions, 3 portal normal, 4 touched -- and two more portal directions).  An error
 * for a batch that keeps none.  Synchronises the batch's stream.  No reference counterpart (diagnostics, bitwise comparisons of two builds). */
int rsim_mpr_records(rsim_batch* b, float* host_out);
/* per candidate pair p (model pair order): out[p] = narrow-phase visits, out[640 + p] = support-function calls (out: 1280 entries), summed over envs and launches since arming */
int rsim_pairlog(rsim_batch* b, unsigned long long* out);

/* zero-copy numpy-view replacement: copy a field to / from HOST float32 (int32 for RSIM_NCON..) buffers of `count` elements */
int rsim_get_array(rsim_batch* b, int field, void* host_dst, size_t count);
int rsim_set_array(rsim_batch* b, int field, const void* host_src, size_t count);
/* device pointer + element count of a field (for DLPack / __cuda_array_interface__ aliasing by the host language) */
void* rsim_device_ptr(rsim_batch* b, int field, size_t* count);
void* rsim_stream(rsim_batch* b);

/* mj_jacSite / mj_jacBody (binding_utils.py:681-695, 826-851) for one env: jacp, jacr are HOST float64 [3,nv], may be NULL.
 * Valid after forward/step1. */
int rsim_jac_site(rsim_batch* b, int env, int site, double* jacp, double* jacr);
int rsim_jac_body(rsim_batch* b, int env, int body, double* jacp, double* jacr);

/* mj_fullM (controllers/parts/controller.py:226-227): dense joint-space inertia of one env, HOST float64 [nv, nv].  Valid after forward / step1 (after a fused
 * control step it is brought up to the current state first, like every derived quantity). */
int rsim_full_M(rsim_batch* b, int env, double* M);
/* sim.data.contact[:ncon] of one env (binding_utils.py:1008-1035; what utils/sim_utils.py:8-40 check_contact and manipulation_env.py:331-376 _check_grasp walk):
 * fills out[0 .. n), returns n = min(ncon, max_out), -1 on error.  geom1 / geom2 are MODEL geom ids; frame = rows {normal (geom1 -> geom2), tangent 1, tangent 2};
 * efc_address = first constraint row of the contact (-1: within the margin but not active); normal_force = constraint force along the normal of the last solve. */
typedef struct rsim_contact {
  double dist, pos[3], frame[9], friction[5], normal_force;
  int32_t geom1, geom2, dim, efc_address;
} rsim_contact;
int rsim_contacts(rsim_batch* b, int env, int max_out, rsim_contact* out);

/* Ray casting against the scene for the whole batch, on the device (csrc/rsim_ray.hip): MuJoCo's mj_ray semantics [3P, docs "API reference: ray collisions"].
 * The result is the nearest surface point at t >= 0 along origin + t dir (dir need not be unit length; t is in units of |dir|); a ray that starts inside a
 * solid reports where it leaves it; a plane is hit only from its +Z side, and a non-zero size[0] / size[1] bounds the hit.  ALL geoms of the model take
 * part, visual ones included; A MESH GEOM IS ITS CONVEX HULL, the geometry this simulator collides with.  A geom is skipped when its rgba alpha is 0, when
 * geomgroup is non-zero and bit `group` of it is clear, when it sits on the world body and flg_static == 0, or when its body is bodyexclude (-1: none).  Ties
 * between geoms go to the lower geom id.  Heightfields are not carried.  The body poses are those of RSIM_XPOS / RSIM_XQUAT (after a fused control step they
 * are brought up to the current state first, like every derived quantity); geom sizes / offsets an env of a per_env_params batch has overridden are honoured.
 * Both calls are asynchronous on the batch's stream, take DEVICE pointers in and out, and allocate nothing after the first of them on a batch (which builds
 * the scene table; a batch that never casts a ray holds none). */
typedef struct { uint32_t geomgroup; int flg_static; int bodyexclude; } rsim_ray_opts;
typedef struct { int body; float pos[3], quat[4]; float fovy_deg; } rsim_camera;   /* pose in the body frame; looks along -Z, +Y up */
/* n_per_env rays per env: origin_dev / dir_dev [B][N][3] -> dist_dev [B][N] (t, -1 = nothing hit), geomid_dev [B][N] (model geom id, -1; may be NULL) */
int rsim_ray(rsim_batch* b, const float* origin_dev, const float* dir_dev, int n_per_env, const rsim_ray_opts* opts, float* dist_dev, int32_t* geomid_dev);
/* One ray per pixel of a pinhole camera, made in the kernel: row r counts from the TOP, the direction of pixel (r, c) in the camera frame is
 * (a tan(fovy / 2) (2 (c + 1/2) / W - 1), tan(fovy / 2) (1 - 2 (r + 1/2) / H), -1) with a = W / H, so depth_dev [B][H][W] is the metric depth along the optical
 * axis (what robosuite's get_real_depth_map yields), +inf where nothing is hit; geomid_dev [B][H][W] (may be NULL) is the `element` segmentation, -1 = none. */
int rsim_render_depth(rsim_batch* b, const rsim_camera* cam, int height, int width, const rsim_ray_opts* opts, float* depth_dev, int32_t* geomid_dev);

/* DynamicsModder / per-episode model edits (utils/mjmod.py:1705-1964, lift.py:311-318): overwrite a float model array
 * (blob field name, e.g. "geom_size", "body_mass", "dof_damping") for envs [env0, env0+nenv). `values` is HOST float64
 * [nenv, count_per_env] in the blob's layout.  Requires per_env_params unless nenv == B with identical rows. */
int rsim_model_param_set(rsim_batch* b, const char* field, int env0, int nenv, const double* values, size_t count_per_env);

/* read back the live value of a float model array (same field names / layout as rsim_model_param_set): HOST float64 [nenv, count_per_env] */
int rsim_model_param_get(rsim_batch* b, const char* field, int env0, int nenv, double* values, size_t count_per_env);

/* Dynamics domain randomisation on the device = DomainRandomizationWrapper(randomize_dynamics) + DynamicsModder.randomize
 * (wrappers/domain_randomization_wrapper.py:47-81,227-259; utils/mjmod.py:1540-1729).  Every call re-draws all enabled parameters of every
 * env RELATIVE TO THE SAVED DEFAULTS (never cumulatively): val = default * (1 + p u) for "ratio" entries, default + p u for "size" entries,
 * u ~ U(-1, 1), then the reference's clips (>= 0; solref in [0, 1]); body quaternions are re-normalised (mjmod.py:1811-1826).
 * Defaults are the float tables at the time of rsim_dr_save_defaults (the wrapper calls save_defaults() after every reset); the on-device
 * episode reset patches defaults and live tables alike.  Draws come from a counter-based generator keyed by (seed, step, env, parameter):
 * the reference uses the unseeded global numpy generator here (mjmod.py:1721), so only the distribution can be matched, not a stream.
 * Requires per_env_params.  A magnitude of 0 disables that parameter. */
typedef struct rsim_dr_desc {
  float density_ratio, viscosity_ratio;                                   /* 0.1, 0.1 */
  float position_size, quaternion_size, inertia_ratio, mass_ratio;        /* 0.0015, 0.003, 0.02, 0.02 */
  float friction_ratio, solref_ratio, solimp_ratio;                       /* 0.1, 0.1, 0.1 */
  float frictionloss_size, damping_size, armature_size;                   /* 0.05, 0.01, 0.01 */
  float stiffness_ratio;                                                  /* 0.1 (domain_randomization_wrapper.py:73,77).  Accepted for completeness: DynamicsModder.mod_stiffness
                                                                           * skips joints whose stiffness is 0 (mjmod.py:1907-1909) and rsim_batch_create refuses models
                                                                           * with joint springs, so there is never a joint for it to act on */
  uint64_t body_mask, geom_mask, joint_mask;                              /* `body_names` / `geom_names` / `joint_names` of the wrapper (:55,64,71) as bit sets: bit b = body id b,
                                                                           * bit g = colliding-geom index g (rsim_model_cgeom), bit j = joint id j; 0 = every body / geom / joint
                                                                           * (the wrapper's None).  Elements outside a subset keep the values they have */
} rsim_dr_desc;
int rsim_dr_save_defaults(rsim_batch* b);
int rsim_randomize_dynamics(rsim_batch* b, const rsim_dr_desc* d, uint64_t seed, uint64_t step);


/* Rollout statistics across the GPUs of a job (SURVEY section 8(b) `rsim_allreduce_stats`, 8(e)): the path's only collective.  Environments are
 * independent worlds, sharded as contiguous blocks over one process per GPU (no data-path exchange); what a training loop sums over ranks once
 * per rollout is a handful of scalars -- env-steps, reward sum, successes, overflow / diverged counts (robosuite itself has no counterpart: its
 * envs are single-process, environments/base.py:23-42).  RCCL (librccl.so, resolved at run time from the process -- the copy PyTorch-ROCm loads --
 * so the library has no link-time dependency on it) over xGMI.
 *   rsim_comm_unique_id   rank 0 draws the 128-byte id (ncclGetUniqueId) and hands it to the other ranks out of band (file, env, torch store ...)
 *   rsim_comm_create      every rank, same id: ncclCommInitRank on `device`; world == 1 is valid (a one-rank communicator)
 *   rsim_allreduce_stats  HOST float64 [n] in, the reduction over all ranks out (op 0 = sum, 1 = max); blocks until the result is on the host
 * The Python host (robosuite_amd/shard.py) uses torch.distributed for the same reduction ("nccl" = RCCL on ROCm, gloo on CPU); this entry is for
 * binders without torch. */
typedef struct rsim_comm rsim_comm;
#define RSIM_COMM_ID_BYTES 128
int rsim_comm_unique_id(void* id_out, size_t bytes);
int rsim_comm_create(const void* id, size_t bytes, int rank, int world, int device, rsim_comm** out);
int rsim_allreduce_stats(rsim_comm* c, double* inout, int n, int op);
void rsim_comm_free(rsim_comm* c);

/* Inverse kinematics of a site for the whole batch, on the device (csrc/rsim_ik.hip): k damped least-squares solves per env, one wavefront each.  Which joint
 * positions of the `ndof` controlled dofs (dof ids, each a hinge or slide joint on the path from the world to the site's body; 1 .. RSIM_JNT_MAX of them)
 * put `site` at the target position and, with target_quat_dev, orientation?  Per iteration: p, R, J = FK(q) (site pose and its Jacobian over the controlled
 * dofs, world frame); err = [p* - p ; w], w the rotation vector of q* (x) conj(q_site), angle in (-pi, pi]; converged when |err_pos| < pos_tol and (with an
 * orientation target) |w| < rot_tol, given up after max_iters updates; A = J J^T + damping I, dq = J^T A^-1 err; with posture_gain > 0 also
 * v = posture_gain (q_rest - q), dq += v - J^T A^-1 (J v), q_rest the start vector; dq scaled so that max |dq| <= max_dq; q += dq, clamped to jnt_range
 * where the joint is limited (clamp_range; the start vector is clamped the same way).  FK is the position stage's (qpos0 offsets, hinge anchors, several
 * joints per body) on the env's OWN model parameters (per_env_params overrides, domain-randomisation draws); a joint on the path that is not controlled is
 * held at the env's current qpos.  A ball joint, a free joint or a mocap body on the path, and a controlled dof that is not on it, fail by name.
 * A PURE QUERY: it reads qpos and the model parameters and writes only its three outputs; state, derived arrays and their stale marks stay as they are.
 * Asynchronous on the batch's stream, DEVICE pointers in and out; the chain table of a (site, dofs) key is built and uploaded by the first call that
 * names it and kept in the batch (a batch that never solves holds none).  q_out of a problem that did not converge is the last iterate: finite and, with
 * clamp_range, inside the ranges.  robosuite_amd/ik.py is the fp64 host mirror. */
typedef struct rsim_ik_opts { float damping, max_dq, pos_tol, rot_tol, posture_gain; int32_t max_iters, clamp_range; } rsim_ik_opts;
/* defaults (opts == NULL): damping 1e-4, max_dq 0.5, pos_tol 1e-4 m, rot_tol 1e-3 rad, posture_gain 0, max_iters 50, clamp_range 1 */
int rsim_ik_site(rsim_batch* b, int site, int ndof, const int32_t* dof_ids, int k,
                 const float* target_pos_dev   /* [B][k][3] */,
                 const float* target_quat_dev  /* [B][k][4] wxyz, or NULL: position only */,
                 const float* q_init_dev       /* [B][k][ndof], or NULL: the env's current qpos */,
                 const rsim_ik_opts* opts      /* NULL: defaults */,
                 float* q_out_dev              /* [B][k][ndof] */,
                 float* err_dev                /* [B][k][2]: |err_pos|, |omega| at q_out (0 without an orientation target) */,
                 int32_t* iters_dev            /* [B][k]: updates made; bit 30 set = converged */);


/* Signed distance and nearest points of geom pairs for the whole batch, on the device (csrc/rsim_dist.hip): MuJoCo's mj_geomDistance [3P, docs "API reference:
 * mj_geomDistance"] for every env and every listed pair.  `pairs` is a HOST array [npair][2] of MODEL geom ids (any geom of the model, visual ones included).
 *   dist     the Euclidean distance of the two solids when they are disjoint and closer than distmax.  A MESH GEOM IS ITS CONVEX HULL; a plane is the infinite
 *            half-space below its +Z face, as in collision.
 *   fromto   the nearest point on geom1, then the nearest point on geom2, world coordinates -- always oriented geom1 to geom2.
 *   status   RSIM_DIST_OK (0): the pair is disjoint and closer than distmax, OR it overlaps and its signed distance is exact: one member is a plane (a plane
 *            against any convex shape, in either slot of the pair), or both members are spheres or capsules.  dist is then minus the penetration depth and
 *            fromto holds the deepest points.
 *            RSIM_DIST_FAR (1): beyond distmax: dist = distmax and fromto is zero (MuJoCo's convention).
 *            RSIM_DIST_OVERLAP (2): any other overlapping pair (box, cylinder, ellipsoid and mesh combinations, and a sphere or capsule against one of them):
 *            dist = 0 and fromto is one common point, twice.  This entry stops at the surface: rsim_geom_distance_signed below returns depth, normal and
 *            witnesses for these pairs, and leaves every other result as it is here; rsim_contacts reports the depth the simulator itself uses.
 *            RSIM_DIST_CAP (bit 8, or-ed in): the iteration stopped at max_iters before its bounds were within tol; dist and fromto are the best iterate,
 *            still a valid upper bound of the distance.
 * Algorithm: GJK on the Minkowski difference of the two cores (a sphere is a point, a capsule a segment; the radii come off at the end); each iteration has an
 * upper and a lower bound on the distance and stops when their gap is <= tol (or fp32 resolves no further progress, which ends it as converged); a plane pair
 * takes no iteration.  Every loop is bounded by max_iters (1 .. RSIM_DIST_MAX_ITERS) or a vertex count.
 * Refused by name (rsim_last_error): a geom id out of range, a geom against itself, plane against plane, a mesh geom whose hull vertices the model does not
 * hold (visual-only meshes: the limit ray casting has), a heightfield, npair < 1.
 * Like rsim_ray: the body poses are those of RSIM_XPOS / RSIM_XQUAT, brought up to the current state first; geom sizes / offsets an env of a per_env_params
 * batch has overridden are honoured; the call is asynchronous on the batch's stream and takes DEVICE pointers for its outputs; it is a pure query of the state.
 * The pair table is uploaded by the first call that names that list and kept in the batch: a repeat call with the same list allocates nothing, and a batch that
 * never asks holds and launches nothing.  robosuite_amd/distance.py is the fp64 host mirror.
 * Not carried: MuJoCo's distance / normal / fromto SENSORS in sensordata, heightfields, a distance term inside IK or the fused step. */
#define RSIM_DIST_OK 0
#define RSIM_DIST_FAR 1
#define RSIM_DIST_OVERLAP 2
#define RSIM_DIST_CAP 256
#define RSIM_DIST_MAX_ITERS 1024
typedef struct rsim_dist_opts { float tol; int32_t max_iters; } rsim_dist_opts;
/* defaults (opts == NULL): tol 1e-6 m on the gap between the iteration's upper and lower bound, max_iters 64.
 * NOTE on tol: status 0 without bit 8 does NOT prove that the two bounds came within tol.  The iteration also ends, as converged, when the support point is one
 * the simplex already holds or the upper bound no longer shrinks in fp32; the lower bound may then still be up to some 1e-4 m below (pairs a few 1e-4 m apart,
 * curved shapes), while dist itself stays within about 1e-6 m of the fp64 value (profiles/distance_parity.txt).  Bit 8 reports the iteration cap only.
 * NOTE on the pair table cache: one device table per distinct pair list is kept until rsim_batch_free, never evicted (as the IK chain tables are); a caller that
 * builds a different list every step should ask for a superset list once instead. */
int rsim_geom_distance(rsim_batch* b, int npair, const int32_t* pairs /* HOST [npair][2] */, float distmax,
                       const rsim_dist_opts* opts /* NULL: defaults */,
                       float* dist_dev            /* [B][npair] */,
                       float* fromto_dev          /* [B][npair][6], or NULL */,
                       int32_t* status_dev        /* [B][npair], or NULL */);

/* rsim_geom_distance with EVERY overlap signed (csrc/rsim_pen.hip k_dist_signed, the per-pair code csrc/rsim_pen_core.h; robosuite_amd/penetration.py is the fp64
 * host mirror and the definition).  A pair rsim_geom_distance does not send to RSIM_DIST_OVERLAP comes back bit for bit as that call returns it.  For the others:
 *   dist     minus the penetration depth: with delta(n) = h_A(n) + h_B(-n), how far geom2 must move along unit n to come free, the depth is a minimum of delta over
 *            the directions and n, the minimiser, the contact normal from geom1 to geom2.
 *   fromto   p1 on geom1's surface in its support set along +n, p2 = p1 + dist n on geom2's supporting plane along -n (MuJoCo's convention for a negative
 *            mj_geomDistance, the one the plane and sphere / capsule pairs follow).  n = (p2 - p1) / dist.
 *   status   RSIM_DIST_OK, or RSIM_DIST_PEN_CAP (bit 9): the descent made pen_iters projections without coming to rest.  The result is then still a valid
 *            DIRECTIONAL depth: dist = -delta(n) for the returned n, an upper bound of the depth.  RSIM_DIST_OVERLAP is never set.
 * Algorithm: a sphere or capsule whose core is apart from the other shape is exact without descent (dist = d_core - r).  Otherwise a descent on the cores: from
 * the direction of least delta among 13 candidates (the centre line, the axes of both geoms), tilted by 1e-3 rad, each step moves geom2 by (delta(n) + offset) n
 * -- outside the Minkowski difference by at least offset -- and runs the GJK of rsim_geom_distance once: the witnesses' direction is the next n, accepted only if
 * delta decreases.  It ends when delta decreases by no more than pen_tol, or not at all, or after pen_iters projections (1 .. RSIM_PEN_MAX_ITERS).
 * LIMITS: what comes out is a LOCAL minimum of the separating translation, never less than the true depth (each face of the Minkowski difference that holds the
 * origin's foot is one; penetration.multistart_depth is the global reference).  Where faces are parallel the witnesses are one point of a face each.  The normal
 * is as good as fp32 resolves a direction over `offset`: depths are within some 1e-4 m of the fp64 mirror, 99 % of them within 1.5e-5 m (profiles/penetration_parity.txt).
 * Refusals, the pair table cache, asynchrony and the pure-query rule are rsim_geom_distance's; in addition a penetration option out of range is refused by name. */
#define RSIM_DIST_PEN_CAP 512
#define RSIM_PEN_MAX_ITERS 128
typedef struct rsim_pen_opts { float pen_tol; int32_t pen_iters; float offset; } rsim_pen_opts;
/* defaults (pen == NULL): pen_tol 1e-7 m, pen_iters 64, offset 4e-3 m (DESIGN.md 5.3 records the choice) */
int rsim_geom_distance_signed(rsim_batch* b, int npair, const int32_t* pairs /* HOST [npair][2] */, float distmax,
                              const rsim_dist_opts* opts /* NULL: defaults */, const rsim_pen_opts* pen /* NULL: defaults */,
                              float* dist_dev            /* [B][npair] */,
                              float* fromto_dev          /* [B][npair][6], or NULL */,
                              int32_t* status_dev        /* [B][npair], or NULL */,
                              int32_t* steps_dev         /* [B][npair] projections made, 0 for a pair that did not descend; or NULL */);

/* Configuration clearance for the whole batch, on the device (csrc/rsim_clear.hip): "is this joint configuration free, and by how much?" for k candidate joint
 * vectors per env -- the body poses at each candidate (rsim_config_fk) and the smallest distance between what the candidate moves and everything it can hit
 * (rsim_config_clearance), without writing the candidate into the state.  What rsim_ik_site returns goes straight in.
 *   candidate   q[env][k][0..ndof): positions of the ndof controlled dofs (dof ids as for rsim_ik_site, 1 .. RSIM_JNT_MAX of them, each of a hinge or slide joint;
 *               they need not lie on one chain: both arms of a two-arm robot in one call is a valid use).  EVERY OTHER JOINT IS HELD AT THE ENV'S CURRENT qpos:
 *               free and ball joints, gripper fingers, objects.  No range clamp: the candidate is evaluated as given.
 *   moved body  a body with a controlled joint on its path to the world; its dof signature is the set of controlled columns on that path.  A body that is not
 *               moved keeps its pose of RSIM_XPOS / RSIM_XQUAT, brought up to the current state first, as every derived read is.
 *   FK          the position stage's: body_pos / body_quat offsets, a hinge about its anchor jnt_pos, a slide along its axis, qpos - qpos0, a held ball joint's
 *               quaternion as it stands -- on the env's OWN float table (per_env_params overrides, domain-randomisation draws), as in rsim_ik_site.
 *   pairs       a HOST list [npair][2] of MODEL geom ids, taken as given: whatever rsim_geom_distance accepts, static pairs included, with its refusals.  Or NULL
 *               with npair 0, THE DEFAULT LIST: the model's collision pairs (pair_geom1 / pair_geom2) whose two bodies have DIFFERENT dof signatures, in the
 *               collision list's order.  That drops the pairs no candidate can change (floor against an object, finger against finger, the last link against
 *               the hand welded to it) and skips, silently, the pairs the distance query refuses (visual-only meshes, heightfields, plane against plane).
 *               rsim_config_pairs returns that list (host only); an empty default list is an error.
 *   result      per (env, k): dist = the minimum over the list of the pair's rsim_geom_distance result at the candidate's poses, by the same rules (signed where
 *               exact, 0 with status 2 for other overlaps, a mesh geom is its convex hull); pair = the index INTO THE LIST of the pair that attains it, the lowest
 *               index on ties; fromto and status are that pair's (RSIM_DIST_CAP or-ed in when its iteration was capped).  With no pair closer than distmax:
 *               dist = distmax, pair = -1, fromto zero, status RSIM_DIST_FAR.
 * Kernels: lane = candidate env * k + j, 64 consecutive candidates per wavefront.  The FK pass leaves the poses of the moved bodies in a scratch the batch owns
 * (grown on demand: a batch that never asks holds none); the distance pass runs a grid of (pair chunks, candidate blocks), each lane handing its running
 * minimum to the pair routine as distmax, so that pairs which cannot beat it leave after an iteration or two; with more than one chunk a last small pass
 * reduces the chunks' partial results in pair order.  opts->chunks forces the chunk count (0: chosen from B * k and the list length).
 * Both device calls are asynchronous on the batch's stream and take DEVICE pointers in and out.  PURE QUERIES: qpos, every derived array and the stale marks stay
 * as they are, but for the refresh a stale derived read always does.  The body table of a dof list and the pair table of a pair list are built and uploaded by
 * the first call that names them and kept in the batch: a repeat call allocates nothing.
 * Refused by name (rsim_last_error): ndof outside 1 .. RSIM_JNT_MAX, a dof id out of range or listed twice, a dof of a free or ball joint, a mocap body among the
 * moved bodies, k < 1, the pair refusals of rsim_geom_distance, an empty default list.
 * A GRASPED OBJECT moves with the candidate only where the caller says so: the _attached entries below (rsim_attach).  In the entries here it is a free body at
 * its current pose.  Not carried: candidates for free or ball joints, a clearance term inside IK or the fused step, heightfields.  (Swept checks along a path:
 * rsim_config_sweep below.)  robosuite_amd/clearance.py is the fp64 host mirror. */
typedef struct rsim_clear_opts { float tol; int32_t max_iters; int32_t chunks; } rsim_clear_opts;   /* NULL: rsim_dist defaults, chunks 0 = automatic */
/* poses of ALL bodies at the candidates (unmoved bodies: the env's current pose) */
int rsim_config_fk(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev /* [B][k][ndof] */,
                   float* xpos_dev /* [B][k][nbody][3] */, float* xquat_dev /* [B][k][nbody][4] wxyz */);
/* the default pair list of a dof list: writes up to max_pairs rows [..][2] of model geom ids, returns the count (-1 on error); host only */
int rsim_config_pairs(const rsim_model* m, int ndof, const int32_t* dof_ids, int max_pairs, int32_t* pairs_out);
int rsim_config_clearance(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev,
                          int npair, const int32_t* pairs /* HOST [npair][2], or NULL with npair 0: the default list */,
                          float distmax, const rsim_clear_opts* opts,
                          float* dist_dev /* [B][k] */, int32_t* pair_dev /* [B][k] */, float* fromto_dev /* [B][k][6] or NULL */, int32_t* status_dev /* or NULL */);

/* Swept clearance for the whole batch, on the device (csrc/rsim_sweep.hip): "is the motion from q0 to q1 free?" for k joint-space segments per env, answered by
 * conservative advancement -- a certificate, not a set of samples: a thin obstacle between two samples is not missed, and a motion far from everything costs a
 * sample or two.
 *   segment     q(t) = q0 + t (q1 - q0), t in [0, 1], for the ndof controlled dofs: q0[env][k][0..ndof), q1 likewise; dof ids, rules and refusals as for
 *               rsim_config_clearance.  EVERY OTHER JOINT IS HELD AT THE ENV'S CURRENT qpos; no range clamp.
 *   clearance   c(t) is exactly what rsim_config_clearance returns for the candidate q(t) over the same pair list (the default list, explicit lists and the
 *               overlap rules carry over) with the same distmax, tol and max_iters, the pair list in one chunk.
 *   bound L     per segment, >= 0: the distance of every listed pair changes by at most L |dt|.  From the env's own float table, in the walk of the body table,
 *               without trigonometry: a moved body carries Omega = the sum of |q1 - q0| over the controlled hinges on its path and V, a bound on the speed of
 *               its origin: V(child) <= V(parent) + Omega(parent) |body_pos|; a slide adds |axis| (|dx| + Omega max(|x(0)|, |x(1)|)) to V (a held slide has
 *               dx = 0, but its current displacement still lengthens the offset); a hinge adds |dq| to Omega and Omega |jnt_pos| to V on either side of its
 *               anchor (a held hinge or ball joint: dq = 0).  A geom moves at most V(b) + Omega(b) r, r = |geom_pos| + a radius about the geom's origin that
 *               contains it (the larger of what its type and geom_size give and |geom_rcenter| + geom_rbound); a geom of a body that is not moved, planes
 *               included, has speed 0.  L = the maximum over the list of the sum of the pair's two bounds, times 1 + 2^-16 for fp32 rounding.
 *               rsim_config_motion_bound returns it (the same device code).  L == 0 (q0 == q1, say): one sample decides.
 *   loop        t = 0; sample c(t); c <= margin + slack: HIT, stop; t == 1: FREE, stop; else t <- min(1, t + (min(c, distmax) - margin) / L) -- a far sample
 *               advances by (distmax - margin) / L; after max_steps samples without a decision: UNDECIDED.
 *   options     margin >= 0 (0), slack > 0 (1e-3 m), max_steps 1 .. RSIM_SWEEP_MAX_STEPS (256): API defaults, not tolerances.  slack is what makes the loop
 *               end: a motion that grazes the scene closer than margin + slack is reported HIT.
 *   result      per (env, k): status = RSIM_SWEEP_FREE (0), RSIM_SWEEP_HIT (1) or RSIM_SWEEP_UNDECIDED (2), RSIM_DIST_CAP (bit 8) or-ed in if the distance
 *               iteration of any sample was capped.  t = 1 for FREE, else the parameter of the last sample: THE MOTION IS CERTIFIED TO HAVE CLEARANCE > margin
 *               ON [0, t).  dist, pair, fromto, t_min: those of the sample with the smallest distance, the earliest on ties (for a HIT the last sample); all
 *               samples far: (distmax, -1, zeros, 0).  steps = the number of samples taken.
 * One kernel, one launch: lane = segment env * k + j, 64 per wavefront, the bound pass and then the loop; a wavefront runs as long as its slowest lane.
 * Asynchronous on the batch's stream, DEVICE pointers in and out, a PURE QUERY; body table, pair table, scratch and the refresh of stale poses are those of
 * rsim_config_clearance: a batch that never sweeps allocates and launches nothing.
 * Refused by name: what rsim_config_clearance refuses; margin < 0, slack <= 0, max_steps out of range, distmax <= margin + slack; a PLANE ON A MOVED BODY (an
 * unbounded solid has no motion bound).
 * NOTE on pairs that stay close: ONE bound L serves the whole list, so a listed pair that sits within margin + slack whatever the dofs do makes every segment a
 * HIT at its first sample, and one that sits just above it holds every step to (its distance - margin) / L.  The Panda's link0 / link1 collision geoms stand
 * 1.0 mm apart at every joint angle: hand in a list without such pairs (parent against child, as a rule).  Per-pair bounds are not carried.
 * A GRASPED OBJECT moves with the motion only where the caller says so: rsim_config_sweep_attached below (rsim_attach); here it is a free body at its current
 * pose.  Not carried: free and ball joints as controlled dofs, interpolation other than linear in joint space, per-pair bounds, a sweep term inside IK or the
 * fused step.  robosuite_amd/sweep.py is the fp64 host mirror. */
#define RSIM_SWEEP_FREE 0
#define RSIM_SWEEP_HIT 1
#define RSIM_SWEEP_UNDECIDED 2
#define RSIM_SWEEP_MAX_STEPS 4096
typedef struct rsim_sweep_opts { float tol; int32_t max_iters; float margin; float slack; int32_t max_steps; } rsim_sweep_opts;
/* defaults (opts == NULL): tol 1e-6, max_iters 64 (rsim_dist_opts), margin 0, slack 1e-3 m, max_steps 256 */
int rsim_config_sweep(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q0_dev /* [B][k][ndof] */, const float* q1_dev /* [B][k][ndof] */,
                      int npair, const int32_t* pairs /* HOST [npair][2], or NULL with npair 0: the default list */,
                      float distmax, const rsim_sweep_opts* opts /* NULL: defaults */,
                      int32_t* status_dev /* [B][k] */, float* t_dev /* [B][k] */, float* dist_dev /* [B][k] */, float* tmin_dev /* [B][k] */,
                      int32_t* pair_dev /* [B][k] */, float* fromto_dev /* [B][k][6] or NULL */, int32_t* steps_dev /* [B][k] or NULL */);
int rsim_config_motion_bound(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q0_dev, const float* q1_dev,
                             int npair, const int32_t* pairs /* as above */, float* bound_dev /* [B][k] */);

/* Carried objects: the five queries above with bodies ATTACHED to links, for the transport half of a pick-and-place.  Each _attached entry is the entry of the
 * same name plus a const rsim_attach*; NULL or n == 0 IS that entry, with its results, its tables and its kernels.
 *   attachment  a pair (body, carrier) of model body ids, up to RSIM_ATTACH_MAX per call, a HOST list like the dof list.  `body` is a child of the world whose
 *               only joint is a free joint (what a robosuite object is); `carrier` is a body the controlled dofs move.  While HELD, body rides rigidly on
 *               carrier: X_body(q) = X_carrier(q) o rel, the quaternion normalised once, as for every walked body.  Its free joint is ignored; the bodies below
 *               it are walked as ordinary moved bodies with their joints held at the env's qpos.
 *   held_dev    DEVICE [B][n] uint8, or NULL: every attachment is held in every env.  An env with 0 treats that body exactly as the plain entries do: a free body
 *               at its current pose, bit for bit (its subtree too).  The caller decides what is grasped; nothing on the device does.
 *   rel_dev     DEVICE [B][n][7], position and wxyz quaternion of body in the carrier's frame ("what if I held it like this", before the grasp exists; the
 *               quaternion is normalised), or NULL: taken in the walk, in fp32, from the env's current RSIM_XPOS / RSIM_XQUAT, brought up to date first as every
 *               derived read is: p_rel = R_c^T (p_b - p_c), q_rel = conj(q_c) q_b.
 *   signature   a held body and its subtree take the carrier's dof signature; not held, they keep their own (empty) one.
 *   pairs       THE DEFAULT LIST with attachments is the model's collision pairs whose two bodies' signatures differ under at least one held row, in the collision
 *               list's order, without the distance query's refusals; rsim_config_pairs_attached returns it.  PER ENV A LISTED PAIR IS EVALUATED ONLY IF ITS TWO
 *               SIGNATURES DIFFER UNDER THAT ENV'S held ROW: a held cube against the fingers that hold it drops out (it would read 0 for ever), a held cube
 *               against the table comes in, and in an env that holds nothing cube against table drops out as it does in the plain entry.  An env that evaluates
 *               no pair reads far.  AN EXPLICIT LIST IS TAKEN AS GIVEN, as in the plain entries: every pair in every env, no skipping.  `pair` in the results
 *               indexes the list handed in or returned.
 *   bound L     a held body has Omega = Omega(carrier) and V = V(carrier) + Omega(carrier) |p_rel|, and its subtree follows by the plain rules; one that is not
 *               held stands still.  L is the maximum over the pairs the env evaluates, times the same 1 + 2^-16.  The certificate carries over unchanged: a held
 *               body's origin is p_c(t) + R_c(t) p_rel with p_rel constant along the motion, so its speed is at most V(carrier) + Omega(carrier) |p_rel| and
 *               its angular speed Omega(carrier) -- the body step's bound with p_rel for body_pos; and the set of evaluated pairs does not depend on t, so c(t) is
 *               L-Lipschitz as before.  A plane on an attached body is refused, as on any moved body.
 * Refused by name, before anything is launched: n outside 0 .. RSIM_ATTACH_MAX or a NULL list; a body id out of range; a body attached twice; a body that is
 * not a world child with exactly one free joint; a mocap body; a free joint, or a controlled joint, anywhere below it; a carrier that is an attached body or
 * below one; a carrier the dof list does not move.
 * The body table's key in the batch is the dof list plus the attachment list: a batch that never names an attachment builds no new table.  A call with
 * attachments runs a second instantiation of the kernels (k_clear_fk_att, k_clear_dist_att, k_sweep_att); the plain kernels are the instantiation with the
 * attachment branches compiled away (the registers and instruction counts they had; the order of the prologue's loads and the size of the kernel argument differ).
 * NOT HANDLED: deciding on the device whether an object is grasped; an object attached to another attached object; attachments in rsim_ik_site, the fused step
 * or rsim_geom_distance; per-env skipping for explicit pair lists; per-pair motion bounds; free or ball joints as controlled dofs; heightfields. */
#define RSIM_ATTACH_MAX 4
typedef struct rsim_attach {
  int32_t n;
  const int32_t* bodies;      /* HOST [n][2]: (body, carrier) */
  const uint8_t* held_dev;    /* DEVICE [B][n], or NULL: all held */
  const float* rel_dev;       /* DEVICE [B][n][7], or NULL: from the env's current poses */
} rsim_attach;
int rsim_config_fk_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, float* xpos_dev, float* xquat_dev, const rsim_attach* att);
int rsim_config_pairs_attached(const rsim_model* m, int ndof, const int32_t* dof_ids, int max_pairs, int32_t* pairs_out,
                               int nattach, const int32_t* attach_bodies /* HOST [nattach][2] */);
int rsim_config_clearance_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs, float distmax,
                                   const rsim_clear_opts* opts, float* dist_dev, int32_t* pair_dev, float* fromto_dev, int32_t* status_dev, const rsim_attach* att);
int rsim_config_sweep_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q0_dev, const float* q1_dev, int npair, const int32_t* pairs,
                               float distmax, const rsim_sweep_opts* opts, int32_t* status_dev, float* t_dev, float* dist_dev, float* tmin_dev, int32_t* pair_dev,
                               float* fromto_dev, int32_t* steps_dev, const rsim_attach* att);
int rsim_config_motion_bound_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q0_dev, const float* q1_dev,
                                      int npair, const int32_t* pairs, float* bound_dev, const rsim_attach* att);
/* how many body tables the batch holds: one per (dof list, attachment list) a config_* call has named so far.  A DIAGNOSTIC, not part of the query contract:
 * it exists so that "a batch that never names an attachment builds no new table" can be checked from outside (tests/test_attach.py); no result depends on it. */
int rsim_config_tables(const rsim_batch* b);

/* Clearance gradients and a collision cost: which way does a candidate move away from the scene?  (rsim_grad.hip; robosuite_amd/clearance.py clearance_grad /
 * collision_cost is the fp64 host mirror; DESIGN.md 5.3 has the derivation.)
 *   rsim_config_clearance_grad (_attached) is rsim_config_clearance (_attached) with one more output, grad_dev [B][k][ndof].  dist, pair, fromto and status are
 *               bit for bit what that entry returns for the same arguments: the same kernels, the same chunking.  fromto_dev and status_dev are needed here (the
 *               gradient is formed from them) and may not be NULL.
 *   grad        for the pair that attains the minimum, with nearest points p1, p2 (fromto), distance d (dist, signed or not) and n = (p2 - p1) / d:
 *                   dd/dq_c = n . (s2_c v_c(p2) - s1_c v_c(p1)),   v_c(p) = a_c x (p - anchor_c) for a hinge, a_c for a slide.
 *               a_c and anchor_c are the world axis and anchor of controlled column c AT THE CANDIDATE, taken in the FK walk at the moment the joint is applied
 *               (axis = R_cur a, anchor = p_cur + R_cur jnt_pos: several joints on one body are right), on the env's own float table.  s_i_c is bit c of the dof
 *               signature of the pair's body i; a held carried body has its carrier's.  No derivative of the witness points enters.  A pair whose two bodies
 *               share a signature needs no special case: its terms cancel.  Negative exact distances (plane, sphere, capsule) take the same formula.
 *   zeros       grad is all zeros where pair < 0 (far), where status has RSIM_DIST_OVERLAP (distance 0, one common point, no direction) and where
 *               |dist| < RSIM_GRAD_MIN_DIST (no usable direction in fp32).
 *   limits      THE DIRECTION IS READ FROM fromto, so its accuracy falls as ulp(coordinate) / |dist| below about a millimetre; and the gradient is ONE-SIDED where
 *               the witnesses are not unique (parallel faces) or the nearest pair ties: it is the derivative of the returned pair at the returned points.
 *   rsim_config_collision_cost (_attached): a smooth cost over ALL near pairs, C1 where the nearest pair switches.  Every listed pair the env evaluates is queried
 *               with distmax = d_safe (no running-minimum pruning).  A pair with d < d_safe adds 1/2 (d_safe - d)^2 to cost_dev [B][k] and -(d_safe - d) grad d,
 *               under the zero rules above, to grad_dev [B][k][ndof]; an overlapping pair (RSIM_DIST_OVERLAP) adds 1/2 d_safe^2 and no gradient and is counted
 *               in noverlap_dev.  nnear_dev counts the contributing pairs.  Either count may be NULL.  Pair lists (default, explicit), attachments, per-env
 *               skipping and refusals are those of rsim_config_clearance (_attached); in addition d_safe <= 0 is refused by name.  With several pair chunks the
 *               partial sums are added in chunk order, without atomics: a repeat call is bit-identical (another chunk count rounds differently).
 * Pure queries, asynchronous on the batch's stream.  They run behind the unchanged clearance kernels (k_clear_fk, k_clear_dist, k_clear_min): k_clear_joints leaves
 * axis and anchor of every controlled column in a store beside the pose scratch, k_clear_grad (_att) writes the gradient of each candidate's own result,
 * k_clear_cost (_att) and k_clear_cost_sum the cost.  The signature table of a dof list and the joint store are built by the first call that asks: a batch that
 * never asks allocates and launches nothing new (rsim_config_grad_tables, a diagnostic like rsim_config_tables, counts the signature tables).
 * The gradient term inside IK is rsim_ik_site_avoid below, which instantiates cost_pairs once more in a code object of its own.
 * NOT HANDLED: a gradient term inside the fused step; penetration depth and gradients for general convex overlaps in THESE entries (their _signed siblings
 * below have them); per-pair outputs (all near
 * pairs with their own gradients); second derivatives; gradients of rsim_config_sweep; free or ball joints as controlled dofs. */
#define RSIM_GRAD_MIN_DIST 1e-7f
int rsim_config_clearance_grad(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs, float distmax,
                               const rsim_clear_opts* opts, float* dist_dev, int32_t* pair_dev, float* fromto_dev, int32_t* status_dev,
                               float* grad_dev /* [B][k][ndof] */);
int rsim_config_clearance_grad_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs, float distmax,
                                        const rsim_clear_opts* opts, float* dist_dev, int32_t* pair_dev, float* fromto_dev, int32_t* status_dev, float* grad_dev,
                                        const rsim_attach* att);
int rsim_config_collision_cost(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs, float d_safe,
                               const rsim_clear_opts* opts, float* cost_dev /* [B][k] */, float* grad_dev /* [B][k][ndof] */,
                               int32_t* nnear_dev /* [B][k] or NULL */, int32_t* noverlap_dev /* [B][k] or NULL */);
int rsim_config_collision_cost_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs, float d_safe,
                                        const rsim_clear_opts* opts, float* cost_dev, float* grad_dev, int32_t* nnear_dev, int32_t* noverlap_dev,
                                        const rsim_attach* att);
int rsim_config_grad_tables(const rsim_batch* b);
/* rsim_config_collision_cost (_attached) with rsim_geom_distance_signed as the pair routine (csrc/rsim_pen.hip k_clear_cost_signed (_att), behind the unchanged
 * k_clear_fk / k_clear_joints and in front of the unchanged k_clear_cost_sum).  An overlapping pair has a direction: it adds 1/2 (d_safe - d)^2 with d < 0 and
 * -(d_safe - d) grad d, by the gradient formula above, and is counted in nnear_dev and in noverlap_dev, which here counts dist < 0.  A candidate without an
 * overlap gets cost, counts and gradient bit for bit as rsim_config_collision_cost returns them (with the same chunk count).  Everything else is that call's.
 * NOT CARRIED: signed distances in rsim_config_sweep: a sweep ends in HIT at margin + slack whatever the sign, and its certificate does not change. */
int rsim_config_collision_cost_signed(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs, float d_safe,
                                      const rsim_clear_opts* opts, const rsim_pen_opts* pen /* NULL: defaults */, float* cost_dev, float* grad_dev,
                                      int32_t* nnear_dev, int32_t* noverlap_dev);
int rsim_config_collision_cost_signed_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs,
                                               float d_safe, const rsim_clear_opts* opts, const rsim_pen_opts* pen, float* cost_dev, float* grad_dev,
                                               int32_t* nnear_dev, int32_t* noverlap_dev, const rsim_attach* att);
/* rsim_config_clearance (_attached) and rsim_config_clearance_grad (_attached) with rsim_geom_distance_signed as the pair routine (csrc/rsim_pen_query.hip
 * k_clear_dist_signed (_att), behind the unchanged k_clear_fk and in front of the unchanged k_clear_min; the gradient entries run the unchanged k_clear_joints /
 * k_clear_grad behind it).  The minimum runs over the SIGNED per-pair values: a colliding candidate reports its deepest listed pair, dist < 0, with that pair's
 * witnesses and status (RSIM_DIST_OK, or with RSIM_DIST_CAP / RSIM_DIST_PEN_CAP; RSIM_DIST_OVERLAP is never set), the lowest pair index on ties; the gradient is
 * the formula above along n = (p2 - p1) / dist and is no longer zero there.  The running minimum is handed to the pair routine as max(minimum, 0), so that an
 * overlapping pair is never taken for far once the minimum is negative; while it is >= 0 the calls are the unsigned entry's: a candidate with no overlapping
 * pair is bit for bit what the unsigned entry returns (with the same chunk count).  Chunk counts agree in dist and pair.  Depths are local minima of the
 * separating translation (rsim_geom_distance_signed's LIMITS).  Pair lists, attachments, per-env skipping, refusals, tables, asynchrony and the pure-query
 * rule are the unsigned entries'; in addition a penetration option out of range is refused by name.  No new tables: rsim_config_tables and
 * rsim_config_grad_tables count what they counted. */
int rsim_config_clearance_signed(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs, float distmax,
                                 const rsim_clear_opts* opts, const rsim_pen_opts* pen /* NULL: defaults */, float* dist_dev, int32_t* pair_dev,
                                 float* fromto_dev, int32_t* status_dev);
int rsim_config_clearance_signed_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs,
                                          float distmax, const rsim_clear_opts* opts, const rsim_pen_opts* pen, float* dist_dev, int32_t* pair_dev,
                                          float* fromto_dev, int32_t* status_dev, const rsim_attach* att);
int rsim_config_clearance_grad_signed(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs, float distmax,
                                      const rsim_clear_opts* opts, const rsim_pen_opts* pen /* NULL: defaults */, float* dist_dev, int32_t* pair_dev,
                                      float* fromto_dev, int32_t* status_dev, float* grad_dev);
int rsim_config_clearance_grad_signed_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int npair, const int32_t* pairs,
                                               float distmax, const rsim_clear_opts* opts, const rsim_pen_opts* pen, float* dist_dev, int32_t* pair_dev,
                                               float* fromto_dev, int32_t* status_dev, float* grad_dev, const rsim_attach* att);

/* Collision-aware inverse kinematics: rsim_ik_site with the collision cost's gradient as a SECONDARY TASK in the null space of the pose task, K problems per env,
 * for the whole batch, on the device (csrc/rsim_ik_avoid.hip; robosuite_amd/ik_avoid.py is the fp64 host mirror and the definition).  The arm's
 * redundancy leaves the obstacle while the site still reaches the target: what repairs a grazing IK solution, as one call.
 *   iteration   per problem q <- clamp(q_init), q_rest = q; then repeat: e, J = the site error and Jacobian exactly as rsim_ik_site defines them (a position-only
 *               target zeroes the angular rows); cost, g, nnear, nover = rsim_config_collision_cost (_attached) at q with the call's pair list, d_safe and
 *               attachments; conv = rsim_ik_site's convergence test, finished = conv and cost <= cost_tol; STOP if finished or after max_iters updates; else
 *               A = J J^T + damping I, v = posture_gain (q_rest - q) - avoid_gain g, dq = J^T A^-1 e + v - J^T A^-1 (J v), scaled so that max |dq| <= max_dq,
 *               q <- clamp(q + dq).  The chain runs max_iters + 1 evaluations; the last one never updates.
 *   cost_tol    every term of the cost is at most the cost, so cost <= 1/2 (d_safe - d_free)^2 proves every listed pair at least d_free apart.  The default
 *               1/2 (d_safe / 2)^2 proves d_free = d_safe / 2 and excludes an overlapping pair (which adds 1/2 d_safe^2).  +inf: never wait for the cost.
 *               (Stopping on nnear == 0 instead would be wrong: the quadratic hinge approaches d_safe asymptotically.)
 *   frozen      a problem that has stopped is frozen: later evaluations of the chain leave every one of its outputs untouched, and its lane leaves the cost
 *               kernel before the pair loop.
 *   outputs     q_out; err, cost and the counts AT q_out; iters = updates made, bit 30 = converged, bit 29 = finished.  q_out of a problem that did not finish
 *               is the last iterate: finite and, with clamp_range, inside the ranges.
 *   check_every c > 0: the host reads one "any problem still running" word after every c evaluations and ends the chain early -- the call then SYNCHRONISES the
 *               stream.  The kernel sets that word with a plain vector store of 1 from every lane that updated; no atomics.  0: fully asynchronous, max_iters + 1
 *               evaluations.  Finished problems are frozen, so both settings return identical bits.
 * Pair lists (pairs HOST [npair][2]; NULL with npair 0, or npair < 0: the default list), attachments (att NULL or n == 0: none), per-env skipping and refusals
 * are rsim_config_collision_cost's; path rules are rsim_ik_site's: a controlled dof that is not on the path to the site is refused by name, so is a ball joint, a
 * free joint or a mocap body on it, and a joint on the path that is not controlled is held at the env's qpos.  Also refused by name: d_safe <= 0,
 * avoid_gain < 0, cost_tol < 0, check_every < 0.
 * A PURE QUERY on each env's own model parameters, on the batch's stream.  Two launches per evaluation (k_ika_cost over (pair chunks, wavefronts), then k_ika_step:
 * the chunk sum, the step and both walks at the new q) behind k_ika_init; rsim_grad.hip, rsim_clear.hip and rsim_ik.hip are untouched.  A batch that never asks
 * allocates and launches nothing new (rsim_ik_avoid_tables, a diagnostic like rsim_config_grad_tables, counts the (site, dofs) keys asked for; the first call of
 * a dof list also uploads that list's signature table, which rsim_config_grad_tables counts).
 * LIMITS: in THIS entry a pair that STARTS in a general convex overlap (status 2) adds cost and no push -- use rsim_ik_site_avoid_signed below, or hand in
 * several start vectors, K > 1; a listed pair that stays inside
 * d_safe whatever the arm does (the Panda's link0 / link1 geoms, 1 mm apart) never lets a problem finish -- hand in the list without parent / child pairs, as for
 * rsim_config_sweep; a 6-dof arm with a pose target has no null space to use.
 * NOT HANDLED: avoidance as a weighted primary task; per-pair active sets between iterations; a sweep or avoidance term inside the fused step; free or ball joints
 * as controlled dofs; compaction of unfinished problems. */
#define RSIM_IK_AVOID_GAIN 100.0f  /* chosen from the fp64 mirror alone on the test scenes: profiles/ik_avoid_parity.txt */
typedef struct rsim_ik_avoid_opts {
  float damping, max_dq, pos_tol, rot_tol, posture_gain; int32_t max_iters, clamp_range;   /* rsim_ik_opts' fields, in its order */
  float d_safe, avoid_gain, cost_tol; int32_t check_every;
} rsim_ik_avoid_opts;
/* defaults (opts == NULL): rsim_ik_opts' (damping 1e-4, max_dq 0.5, pos_tol 1e-4 m, rot_tol 1e-3 rad, posture_gain 0, max_iters 50, clamp_range 1), d_safe 0.05,
 * avoid_gain RSIM_IK_AVOID_GAIN, cost_tol 1/2 (d_safe / 2)^2, check_every 0 */
int rsim_ik_site_avoid(rsim_batch* b, int site, int ndof, const int32_t* dof_ids, int k,
                       const float* target_pos_dev   /* [B][k][3] */,
                       const float* target_quat_dev  /* [B][k][4] wxyz, or NULL: position only */,
                       const float* q_init_dev       /* [B][k][ndof], or NULL: the env's current qpos */,
                       int npair, const int32_t* pairs /* HOST [npair][2]; NULL with npair 0, or npair < 0: the default list */,
                       const rsim_ik_avoid_opts* opts /* NULL: defaults */, const rsim_clear_opts* clear_opts /* NULL: defaults */,
                       const rsim_attach* att        /* or NULL */,
                       float* q_out_dev              /* [B][k][ndof] */,
                       float* err_dev                /* [B][k][2]: |err_pos|, |omega| at q_out */,
                       int32_t* iters_dev            /* [B][k]: updates made; bit 30 = converged, bit 29 = finished */,
                       float* cost_dev               /* [B][k]: the collision cost at q_out */,
                       int32_t* nnear_dev            /* [B][k] or NULL */, int32_t* noverlap_dev /* [B][k] or NULL */);
int rsim_ik_avoid_tables(const rsim_batch* b);
/* rsim_ik_site_avoid with rsim_config_collision_cost_signed as the cost of every evaluation (csrc/rsim_pen_query.hip k_ika_cost_signed (_att) in front of the
 * unchanged k_ika_step, behind the unchanged k_ika_init): a pair that starts in a general convex overlap has a depth and a normal, so it pushes, and a problem
 * whose start vector sits in an overlap with its target already reached moves out through the null space instead of standing still for max_iters evaluations.
 * noverlap_dev counts dist < 0.  With avoid_gain 0 and cost_tol +inf, q_out, err and iters are rsim_ik_site_avoid's bit for bit.  Everything else is that
 * call's (it takes att itself: no _attached twin); in addition a penetration option out of range is refused by name.  rsim_ik_avoid_tables counts its keys
 * as that call's. */
int rsim_ik_site_avoid_signed(rsim_batch* b, int site, int ndof, const int32_t* dof_ids, int k, const float* target_pos_dev, const float* target_quat_dev,
                              const float* q_init_dev, int npair, const int32_t* pairs, const rsim_ik_avoid_opts* opts, const rsim_clear_opts* clear_opts,
                              const rsim_pen_opts* pen /* NULL: defaults */, const rsim_attach* att, float* q_out_dev, float* err_dev, int32_t* iters_dev,
                              float* cost_dev, int32_t* nnear_dev, int32_t* noverlap_dev);

/* Dynamics at candidate configurations: "can the arm hold or execute this?" -- joint torques, the joint-space inertia and a site Jacobian at k candidate joint
 * vectors per env, for the whole batch, on the device (csrc/rsim_dyn.hip; robosuite_amd/dynamics.py is the fp64 statement by the definition).
 * Candidates, controlled dofs, refusals, the env's OWN float table (per_env_params overrides, domain-randomisation draws) and the pure-query rules are
 * rsim_config_fk's, word for word: ndof is 1 .. RSIM_JNT_MAX dof ids of hinge or slide joints, which need not lie on one chain; every other joint is held at the
 * env's current qpos; no range clamp; a batch that never asks allocates and launches nothing.
 * In addition EVERY JOINT THAT IS NOT CONTROLLED HAS ZERO VELOCITY AND ZERO ACCELERATION.  With q~ the env's qpos with the controlled entries replaced, and qd~ /
 * qdd~ zero but for the controlled entries:
 *   rsim_config_inverse_dynamics   tau[c] = (M(q~) qdd~)[dof_c] + qfrc_bias(q~, qd~)[dof_c] + dof_damping[dof_c] * qd_c.  M includes dof_armature; qfrc_bias is
 *               MuJoCo's: Coriolis, centrifugal and gravity, gravity from the env's own opt table.  qd_dev / qdd_dev may each be NULL (zeros): with both NULL the
 *               result is the gravity torque.  Only moved bodies contribute -- held gripper bodies that ride on the arm are moved bodies.
 *               NOT INCLUDED: tendon springs and dampers, fluid forces, friction loss, actuator, contact, equality and applied forces.  (Joint springs cannot
 *               occur: rsim_batch_create refuses them.)
 *   rsim_config_mass_matrix        the block of M(q~) on the controlled dofs, [B][k][ndof][ndof]: the inertia of the mechanism with all other joints locked.  Both
 *               triangles are written and are equal bit for bit; two columns on different branches give exactly 0.
 *   rsim_config_jacobian           mj_jacSite at the candidate in the controlled columns, [B][k][3][ndof] each (either output may be NULL, not both); the site is
 *               placed from the env's own site_pos on its body's candidate pose.  A site on a body no controlled dof moves is valid and reads zeros.
 * Kernels: behind the unchanged k_clear_fk and k_clear_joints, which leave the moved bodies' poses and the controlled joints' world axes and anchors, ONE kernel
 * each, lane = candidate: k_dyn_rne (recursive Newton-Euler: a forward and a backward walk of the body table), k_dyn_crb (composite rigid bodies) and k_dyn_jac.
 * Moments are taken about the candidate's position of the first moved body, not the world origin.  Per-body words live in a batch scratch grown on demand; a lane
 * touches only its own words: no atomics, a repeat call is bit-identical.  Asynchronous on the batch's stream, DEVICE pointers in and out.
 * Refused by name: what rsim_config_fk refuses, a NULL output, and for the Jacobian a site out of range.
 * NOT CARRIED: free or ball joints as controlled dofs; body or point Jacobians other than sites; a torque-limit term inside IK or
 * the fused step; tendon and fluid terms.  (Forward dynamics at candidates: rsim_config_forward_dynamics below; the payload of carried objects: the _attached
 * entries at the end of this file.) */
int rsim_config_inverse_dynamics(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev /* [B][k][ndof] */,
                                 const float* qd_dev /* [B][k][ndof] or NULL: zeros */, const float* qdd_dev /* likewise */, float* tau_dev /* [B][k][ndof] */);
int rsim_config_mass_matrix(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, float* M_dev /* [B][k][ndof][ndof] */);
int rsim_config_jacobian(rsim_batch* b, int site, int ndof, const int32_t* dof_ids, int k, const float* q_dev,
                         float* jacp_dev /* [B][k][3][ndof] or NULL */, float* jacr_dev /* likewise */);

/* M^-1 at candidate configurations: "what acceleration does this torque give here, what is the end effector's apparent inertia here?" -- the other half of the
 * dynamics queries above, on the device (csrc/rsim_dyn_solve.hip; robosuite_amd/dynamics.py forward_dynamics / mass_solve / opspace is the fp64 statement;
 * DESIGN.md 5.3).  Candidates, controlled dofs, refusals, the env's OWN float table and the pure-query rules are rsim_config_fk's, word for word, as for
 * rsim_config_mass_matrix; M below is that call's block: the inertia of the mechanism with every other joint locked, at zero velocity and acceleration.
 *   rsim_config_forward_dynamics   qdd = M(q~)^-1 (tau - qfrc_bias(q~, qd~) - dof_damping qd), [B][k][ndof]: the bias and damping terms are exactly what
 *               rsim_config_inverse_dynamics returns with qdd_dev NULL.  qd_dev / tau_dev may each be NULL (zeros).  The exact inverse of
 *               rsim_config_inverse_dynamics, with its limits: NOT INCLUDED are tendon, fluid, friction-loss, actuator, contact, equality and applied forces.
 *   rsim_config_mass_solve         x = M(q~)^-1 rhs for rhs [B][k][ndof][nrhs], 1 <= nrhs <= RSIM_JNT_MAX; x has rhs's shape.
 *   rsim_config_opspace            with J = [jacp; jacr] of rsim_config_jacobian (6 x ndof): minv_jt = M^-1 J^T [B][k][ndof][6] and lambda_inv = J M^-1 J^T
 *               [B][k][6][6].  Each unordered pair of lambda_inv is computed once and written to both triangles: symmetric bit for bit.  Either output may be
 *               NULL, not both.  The operational-space inertia Lambda itself is NOT returned: lambda_inv is singular for ndof < 6 and at kinematic singularities,
 *               and robosuite takes its pseudo-inverse -- Lambda = pinv(lambda_inv), Jbar = minv_jt Lambda are two lines for the caller.
 * ok_dev, int32 [B][k] or NULL: 1 where every pivot of the Cholesky factorisation of M was finite and > 0.  Where it is 0 that candidate's outputs are NaN; no
 * other candidate is affected.
 * Kernels: the unchanged k_clear_fk, k_clear_joints, k_dyn_crb (and k_dyn_rne with qdd NULL, or k_dyn_jac), writing into batch scratches grown on demand, then
 * ONE kernel k_dyn_solve, lane = candidate, one wavefront per workgroup: the lane's packed lower triangle and one right-hand-side column in dynamic LDS laid out
 * [word][lane] ((ndof (ndof + 1) / 2 + ndof) * 256 B per workgroup), Cholesky in place, forward and back substitution per column.  A lane touches only its own
 * words: no barrier, no atomics, a repeat call is bit-identical.  A block-diagonal M (two arms) factorises to a block-diagonal L exactly.  Asynchronous on the
 * batch's stream, DEVICE pointers in and out.  A batch that never asks allocates and launches nothing.
 * Refused by name: what rsim_config_fk refuses, a NULL output (for rsim_config_opspace: both NULL), nrhs out of range, a site out of range.
 * NOT CARRIED: Lambda or pseudo-inverses; free or ball joints as controlled dofs; constraint, contact or actuator forces in the
 * acceleration; integrating candidates forward in time.  (Derivatives: rsim_config_forward_dynamics_grad at the end of this file.) */
int rsim_config_forward_dynamics(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev /* [B][k][ndof] */,
                                 const float* qd_dev /* [B][k][ndof] or NULL: zeros */, const float* tau_dev /* likewise */, float* qdd_dev /* [B][k][ndof] */,
                                 int32_t* ok_dev /* [B][k] or NULL */);
int rsim_config_mass_solve(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int nrhs, const float* rhs_dev /* [B][k][ndof][nrhs] */,
                           float* x_dev /* [B][k][ndof][nrhs] */, int32_t* ok_dev /* [B][k] or NULL */);
int rsim_config_opspace(rsim_batch* b, int site, int ndof, const int32_t* dof_ids, int k, const float* q_dev, float* lambda_inv_dev /* [B][k][6][6] or NULL */,
                        float* minv_jt_dev /* [B][k][ndof][6] or NULL */, int32_t* ok_dev /* [B][k] or NULL */);

/* Carried payloads in the dynamics queries: "is this executable WITH THE OBJECT IN HAND?" -- the six entries above with bodies ATTACHED to links
 * (csrc/rsim_dyn_att.hip; robosuite_amd/dynamics.py with attach / held / rel is the fp64 statement).  Each _attached entry is the entry of the same
 * name plus a trailing const rsim_attach*; NULL or n == 0 IS that entry, with its results, its tables and its kernels.  The attachment rules are rsim_attach's,
 * unchanged: up to RSIM_ATTACH_MAX pairs (body, carrier), held_dev [B][n] or NULL (all held), rel_dev [B][n][7] or NULL (the env's current poses), the same
 * refusals by name, plus the plain entry's own.
 * In an env whose held row holds attachment i:
 *   - the attached body and every body below it are RIGID LOAD on the carrier, at X_carrier(q) o rel; the joints below are held at the env's qpos, as in FK.
 *   - each such body has the carrier's velocity and acceleration and contributes its wrench to tau and its inertia to M, through the carrier's dof signature (the
 *     held half of the signature word).  Nothing else sees them.
 *   - masses, inertias, ipos and iquat are the env's OWN tables: two envs with the same grasp and a different body_mass get different torques.
 *   - the free joint of the attached body has no column and no armature: it is ignored, as in FK.
 * In an env that does not hold attachment i its bodies contribute nothing, and EVERY OUTPUT OF THAT ENV IS BIT FOR BIT WHAT THE PLAIN ENTRY RETURNS.
 * Site Jacobians (rsim_config_jacobian_attached, rsim_config_opspace_attached): the site may sit on an attached body or below one.  Held: the point is placed
 * from the attached pose and the columns are the carrier's signature.  Not held: zeros, the rule for a site no controlled dof moves.
 * rsim_config_forward_dynamics_attached is the exact inverse of rsim_config_inverse_dynamics_attached with the same attachment.
 * Kernels: behind k_clear_fk_att and the unchanged k_clear_joints, ONE kernel each, lane = candidate: k_dyn_rne_att, k_dyn_crb_att, k_dyn_jac_att -- the walks of
 * the plain kernels in which a held attached body takes V and A from its carrier's slot and adds its wrench / inertia there (moments are about one fixed point,
 * so they add); where the env does not hold it the slot is stored as zero and nothing is added.  k_dyn_solve runs unchanged behind them.  The dynamics scratch
 * is sized by the table's slots, which count the attached ones.  A lane touches only its own words: no atomics, a repeat call is bit-identical.  A batch that
 * never names an attachment in a dynamics call builds no new table, launches no new kernel and allocates nothing new.
 * NOT CARRIED: a virtual payload with no body in the model; deciding on the device what is grasped; contact or grasp forces between hand and object; attachments
 * in rsim_ik_site; an object attached to an attached object; free or ball joints as controlled dofs; derivatives. */
int rsim_config_inverse_dynamics_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, const float* qd_dev, const float* qdd_dev,
                                          float* tau_dev, const rsim_attach* att);
int rsim_config_mass_matrix_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, float* M_dev, const rsim_attach* att);
int rsim_config_jacobian_attached(rsim_batch* b, int site, int ndof, const int32_t* dof_ids, int k, const float* q_dev, float* jacp_dev, float* jacr_dev,
                                  const rsim_attach* att);
int rsim_config_forward_dynamics_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, const float* qd_dev, const float* tau_dev,
                                          float* qdd_dev, int32_t* ok_dev, const rsim_attach* att);
int rsim_config_mass_solve_attached(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, int nrhs, const float* rhs_dev, float* x_dev,
                                    int32_t* ok_dev, const rsim_attach* att);
int rsim_config_opspace_attached(rsim_batch* b, int site, int ndof, const int32_t* dof_ids, int k, const float* q_dev, float* lambda_inv_dev, float* minv_jt_dev,
                                 int32_t* ok_dev, const rsim_attach* att);

/* Derivatives of the dynamics at candidate configurations: "how do the torques, and the accelerations, change with the configuration and its rate?" -- the
 * analytic first derivatives of rsim_config_inverse_dynamics and rsim_config_forward_dynamics, on the device (csrc/rsim_dyn_grad.hip; robosuite_amd/dynamics.py
 * inverse_dynamics_grad / inverse_dynamics_jvp / forward_dynamics_grad is the fp64 statement by the definition of a derivative).  Candidates,
 * controlled dofs, refusals, the env's OWN float table and the pure-query rules are rsim_config_fk's, word for word, with the entry's own name in the message;
 * every joint that is not controlled is held with zero velocity and acceleration, as for rsim_config_inverse_dynamics, and is no direction of differentiation.
 *   rsim_config_inverse_dynamics_grad   tau [B][k][ndof], bit for bit rsim_config_inverse_dynamics's (it is that kernel's output), and
 *               dtau_dq, dtau_dqd [B][k][ndof][ndof], entry [i][j] = d tau_i / d q_j (resp. qd_j) at (q, qd, qdd).  d tau / d qdd is M: rsim_config_mass_matrix.
 *   rsim_config_inverse_dynamics_jvp    dtau [B][k][ndof] = dtau_dq dq + dtau_dqd dqd + M dqdd for one direction per candidate, in one walk; dq_dev, dqd_dev and
 *               dqdd_dev may each be NULL (zeros).  It agrees with the product of the blocks within rounding, not bit for bit.
 *   rsim_config_forward_dynamics_grad   qdd and ok exactly rsim_config_forward_dynamics's chain and bits; dqdd_dq = -M^-1 dtau_dq and dqdd_dqd = -M^-1 dtau_dqd,
 *               both taken AT (q, qd, qdd), [B][k][ndof][ndof].  d qdd / d tau is M^-1: rsim_config_mass_solve of the identity; it is not returned here.  Where
 *               ok is 0 the candidate's three outputs are NaN; no other candidate is affected.
 * The joint angle turns about the NORMALISED stored axis while a column uses the stored axis itself: the device differentiates with the stored one, so column j of
 * d / dq differs from the derivative of the statement by the factor |axis_j|, within about 2^-23 of 1.
 * Kernels: behind the unchanged k_clear_fk, k_clear_joints and k_dyn_rne (at the point of linearisation), lane = candidate: k_dyn_rne_jvp, one tangent
 * (forward-mode) Newton-Euler walk, or k_dyn_rne_grad, the 2 ndof unit directions in a loop inside the lane, with a flag that writes minus the blocks for the
 * forward-dynamics chain; that chain then runs the unchanged k_dyn_solve on each block in place.  Tangent words (24 per moved body and candidate) live in a batch
 * scratch of their own, grown on demand and reused from direction to direction.  A lane touches only its own words: no atomics, a repeat call is
 * bit-identical.  Asynchronous on the batch's stream, DEVICE pointers in and out.  A batch that never asks allocates and launches nothing new.
 * Refused by name: what rsim_config_fk refuses, a NULL output.
 * NOT CARRIED: attachments; second derivatives; derivatives with respect to model parameters; free or ball joints as controlled dofs; derivatives of
 * rsim_config_opspace or rsim_config_jacobian; a reverse-mode kernel (the vector-Jacobian product is a contraction of the ndof x ndof blocks); any use inside
 * the fused step or rsim_ik_site. */
int rsim_config_inverse_dynamics_grad(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev /* [B][k][ndof] */,
                                      const float* qd_dev /* [B][k][ndof] or NULL: zeros */, const float* qdd_dev /* likewise */, float* tau_dev /* [B][k][ndof] */,
                                      float* dtau_dq_dev /* [B][k][ndof][ndof] */, float* dtau_dqd_dev /* likewise */);
int rsim_config_inverse_dynamics_jvp(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, const float* qd_dev, const float* qdd_dev,
                                     const float* dq_dev /* [B][k][ndof] or NULL: zeros */, const float* dqd_dev /* likewise */, const float* dqdd_dev /* likewise */,
                                     float* dtau_dev /* [B][k][ndof] */);
int rsim_config_forward_dynamics_grad(rsim_batch* b, int ndof, const int32_t* dof_ids, int k, const float* q_dev, const float* qd_dev /* or NULL */,
                                      const float* tau_dev /* or NULL */, float* qdd_dev /* [B][k][ndof] */, float* dqdd_dq_dev /* [B][k][ndof][ndof] */,
                                      float* dqdd_dqd_dev /* likewise */, int32_t* ok_dev /* [B][k] or NULL */);

#ifdef __cplusplus
}
#endif
#endif
