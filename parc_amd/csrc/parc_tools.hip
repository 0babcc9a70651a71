// parc_tools.hip -- the stage-2 motion tools and the learner's kernels of include/parc_env.h as one translation unit, apart from the env
// (parc_env.hip) and the dynamics (parc_dynamics.hip).
// Every header includes what it uses; the order below does not matter.  The first four are what the tools share; no tool header
// includes another tool's, but for the path rollout, which runs the generator, the rollout selection, which reads the path handle's
// scene and scores with the analyser's SDF search, and the contact labelling, which takes the analyser's cell SDF and linspace centres.
#include "parc_char.hpp"             // the character as the motion tools see it: CharTree / CharPoints, fk_frame, the vector helpers
#include "parc_grid.hpp"             // heightfield helpers of more than one tool: to_i64, grid_index, sd_box
#include "parc_clip_batch.hpp"       // the clip batch: the device views ClipArrays / FrameClips, validation and upload
#include "parc_tool_handle.hpp"      // the host skeleton of a handle: checked launch, create, slots, state guards, status words, kernel times
#include "parc_motion_opt.hpp"       // parc_mopt_*: the batched kinematic motion optimiser
#include "parc_motion_terrain.hpp"   // parc_mterr_*: motion-terrain analysis
#include "parc_motion_edit.hpp"      // parc_medit_*: stage 2's hesitation-frame removal
#include "parc_motion_label.hpp"     // parc_mlabel_*: contact labelling, penetration lift and resampling of raw clips (uses the analyser's cell SDF)
#include "parc_motion_sampler.hpp"   // parc_msamp_*: the generator's motion-window sampler
#include "parc_path_planner.hpp"     // parc_pathplan_*: stage 2's batched A* terrain path planner
#include "parc_terrain_gen.hpp"      // parc_tgen_*: stage 2's BOXES / PATHS / STAIRS terrain generators, batched
#include "parc_motion_aug.hpp"       // parc_maug_*: stage 0's motion-terrain augmenter and the mirrored copies, batched
#include "parc_mdm.hpp"              // parc_mdm_*: the motion generator's inference, the MDM denoiser and its DDIM / DDPM loops
#include "parc_mdm_path.hpp"         // parc_mpath_*: path-following generation, the generator's world-frame wrapper and the rollout along a path
#include "parc_mpath_select.hpp"     // parc_msel_*: the rollout's selection, rows scored on their own terrain slices, filtered and ranked (uses the analyser's SDF)
#include "parc_mdm_loss.hpp"        // parc_mloss_*: the motion generator's training loss, the thirteen terms and their gradient in one launch
#include "parc_learner.hpp"          // parc_td_lambda_return, parc_normalize_record, parc_gather_rows: the learner's kernels
