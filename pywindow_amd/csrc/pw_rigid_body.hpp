// pw_rigid_body.hpp -- the pose-averaged affinity of a cavity for a rigid guest that is a body, not a line
// (include/pywindow_amd.h: pw_rigid_body_affinity), single source for the gfx950 kernels (pw_rigid_body.hip) and the host
// path (pw_hostpath.cpp).  Everything but the site position is pw_rigid.hpp's and pw_affinity.hpp's; this file adds the
// position of a site read from a table.  The reference has no counterpart.
//
// DEFINED RESULT.  A job has the grid, the REGION, core2, cutoff2, the L betas, the n atoms X, the rows (A, B, C) per
//     (site, atom) and `charged` of a pw_rigid_affinity job.  It has no offsets and no directions.  It has a POSE TABLE:
//     M * S rows of three doubles, 1 <= M <= RIGID_MAX_DIRS and 1 <= S <= RIGID_MAX_SITES; row o * S + s is the
//     displacement p_{o,s} of site s from the guest's centre in pose o; every component finite with
//     |component| <= RIGID_MAX_OFFSET (16).  The rows are data: nothing orthogonalises them, checks them or rotates
//     them.  The kernel knows nothing of rotations.
//   POSE (v, o)  voxel v has the centre (x, y, z) by cavity_coord.  Site s sits at px = x + p_{o,s}.x, likewise py and
//            pz: one rounded sum a coordinate (rigid_body_site).  Everything after that is pw_rigid.hpp's POSE: per site
//            the atoms in index order, aff_r2, aff_blocked, aff_counts, rigid_pair<CHARGED>, per-site accumulators from
//            +0.0, then U = U_0 + U_1 + ...
//   WEIGHT, VOXEL, SUMS, WRITTEN  pw_rigid.hpp's: aff_weight with its clamp, RigidFold over o in order, inv_M, umin_v by
//            strict < in o order, dead voxels, the chunk tree, the partial of rigid_part_words(L) words, the reduce.
//            min_dir of pw_rigid_out is the pose index o.
//
// PROOF OBLIGATIONS.
//   (1) Linear guests are a special case, to the byte.  The table p_{o,s} = (t_s * d_o.x, t_s * d_o.y, t_s * d_o.z), one
//       rounded product each, gives every output of pw_rigid_affinity for the offsets t and the directions d:
//       rigid_site(x, t, d) is that product followed by that sum, and rigid_body_site(x, t * d) is that sum; no other
//       statement of the two definitions differs.  |t * d| <= 16 follows from |t| <= 16 and |d| <= 1.
//   (2) The table may hold anything rigid per pose.  The definition uses no relation between the rows of two poses or
//       between the rows of one pose, so a rotation set of one conformer and several conformers of a flexible guest,
//       each in its rotations, are the same call.  (Only the first is a public use of the library.)
//   (3) No result shows how the table reaches the arithmetic: the kernel brings RIGID_BODY_POSE_BLOCK poses into LDS at
//       a time and evaluates RB of them a pass; a pose's energy depends on its own rows only, and the fold takes the
//       poses in o order whatever the block and RB are.
#pragma once
#include "pw_rigid.hpp"

namespace pw {

constexpr int RIGID_BODY_POSE_BLOCK = 64;            // poses whose displacements are in LDS at a time (a multiple of every RB)

// a coordinate of a site: the centre's plus the displacement's component, one rounded sum
PW_HD inline double rigid_body_site(double x, double p) { return x + p; }

}  // namespace pw
