// myo_host_tasks.h -- the table of all tasks: every myo_task_<name>.h, the lookup of a task's hook record and the observation launch that
// goes through it.  A new task is its file, its #include here and its row in task_hooks.  The file holds the task's row record (the
// blocks of its canonical observation row, each width once), the observation body that writes through it, the configure that takes obs_dim
// from it, the reward column names, the observation-term table built from it, and the hook record that hands all of these to the host:
// myo_rewards.h and myo_obs_terms.h look a task's tables up through task_hooks and name no task.  (The walk row is written inside the step
// kernel, so its record sits beside DevWalk in myo_common.h.)  On the Python side the task adds its setup to tasks.py, its reward keys to
// rewards.py and its term names and width expressions to observations.py; tests/test_obs_terms_host.py holds those to the tables here by value.
#ifndef MYO_HOST_TASKS_H
#define MYO_HOST_TASKS_H

#include "myo_task_util.h"
#include "myo_task_pose.h"
#include "myo_task_reach.h"
#include "myo_task_walk.h"
#include "myo_task_stand.h"
#include "myo_task_hold.h"
#include "myo_task_keyturn.h"
#include "myo_task_pen.h"
#include "myo_task_baoding.h"
#include "myo_task_die.h"
#include "myo_task_myodm.h"
#undef RWD_TAIL
#undef RWD_COLS
#undef ROW
#undef TERM

static const TaskHooks* task_hooks(int task) {
  switch (task) {
    case MYO_TASK_POSE: return &pose_hooks;
    case MYO_TASK_REACH: return &reach_hooks;
    case MYO_TASK_WALK: return &walk_hooks;
    case MYO_TASK_STAND: return &stand_hooks;
    case MYO_TASK_HOLD: return &hold_hooks;
    case MYO_TASK_TRACK: return &track_hooks;
    case MYO_TASK_KEYTURN: return &keyturn_hooks;
    case MYO_TASK_PEN: return &pen_hooks;
    case MYO_TASK_BAODING: return &baoding_hooks;
    case MYO_TASK_DIE: return &die_hooks;
    default: return nullptr;   // MYO_TASK_NONE
  }
}

static int launch_obs(myo_batch* b, hipStream_t s, int obs_only = 0, int reset_only = 0) {
  const TaskHooks* hooks = task_hooks(b->task.task);
  if (!hooks) return fail(MYO_E_ARG, "myo_obs: no task configured");
  const int rc = hooks->obs(b, s, obs_only, reset_only);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

#endif  // MYO_HOST_TASKS_H
