"""mcba -- MI355X-native bundle adjustment behind the reference's `bundle_adjust()`.

Only what the hot path needs lives here:
  csrc/      HIP kernels for gfx950 + the C-ABI (`libmcba.so`, declared in include/mcba.h)
  build.py   hipcc driver that compiles csrc/ in-tree
  ops.py     ctypes binding of that ABI (fails loudly if the library is missing)
  solver.py  host-side Levenberg-Marquardt / Schur driver
  api.py     `bundle_adjust` with the reference's exact signature and return tuple
  diagnostics.py  reprojection_errors (numeric core of plot_residuals), undistort_points -- SURVEY.md section 8f-2
  flatibration.py  get_floor_points / flatibrate / center_arena / flip_z_axis (floor-plane alignment) -- SURVEY.md section 8f-5
  detection.py  detect_chessboard / detect_chessboards / reorder_chessboard_corners and the reference's host helpers -- SURVEY.md section 8f-7
  io.py      save_calibration / load_calibration (json, jarvis; gimbal needs h5py) -- SURVEY.md section 8f-3
  geometry.py  project_points / project_to_cameras / apply_rigid_transform / keypoint_reprojection_errors / refine_triangulation and the reference's matrix helpers -- SURVEY.md section 8f-8;
             triangulate_consensus (per-detection inlier masks) -- SURVEY.md section 8f-9;
             refine_extrinsics (free-point bundle adjustment of the extrinsics on keypoint detections) -- SURVEY.md section 8f-12;
             estimate_relative_pose / extrinsics_from_keypoints (two-view RANSAC and a scale chain: extrinsics from keypoints alone; solver="5point" for thin scenes) -- SURVEY.md sections 8f-14, 8f-17;
             refine_cameras (refine_extrinsics with free intrinsics and a Gaussian prior on them: 12 unknowns per camera, 2 to 12 cameras) -- SURVEY.md section 8f-15;
             resect_camera / resect_cameras (resection: a camera's pose from known 3-D points and its own detections -- PnP RANSAC and a pose-only polish) -- SURVEY.md section 8f-16;
             solver="p3p" on either (a minimal 3-point generator for coplanar or nearly coplanar points and for heavy outlier shares) -- SURVEY.md section 8f-18
  uncertainty.py  calibration_uncertainty (parameter covariance from the Schur system) -- SURVEY.md section 8f-10;
             triangulation_uncertainty (covariance of every triangulated point) -- SURVEY.md section 8f-11
             weights= on refine_triangulation / triangulate(refine=True) / triangulation_uncertainty / refine_extrinsics (per-detection confidence
             weights: a detection of weight w enters the cost as if it and fx, fy, cx, cy of its camera were multiplied by sqrt(w)) -- SURVEY.md section 8f-13
  trajectory.py  smooth_trajectories (the fixed-interval smoother of keypoint tracks: gaps filled, every frame trusted as its covariance says,
             gross errors discounted by a robust loss) -- SURVEY.md section 8f-19; trajectory_uncertainty (the covariance of every
             smoothed point and of neighbouring frames, by selected inversion) -- section 8f-20; refine_trajectories (the tracks refined on
             the raw detections: Gauss-Newton on the reprojection cost plus the smoothness prior, single-camera frames used) -- section 8f-21;
             estimate_accel_std and trajectory_evidence (accel_std from the tracks themselves: the maximum of the smoother's evidence) -- section 8f-24
  skeleton.py  refine_skeleton (the keypoints of a frame refined together, joined by bones of known length: a keypoint one camera saw is located,
             the others get tighter) and estimate_bone_lengths (exact medians of the bone lengths and their spread) -- SURVEY.md section 8f-22; refine_skeleton_trajectories (the tracks of a recording refined together: the
             detections, the time prior and the bones in one fit, conjugate gradients preconditioned by the smoother's elimination) -- section 8f-23
  synth.py   deterministic synthetic board detections for tests and bench
"""
from . import synth  # noqa: F401
from . import ops, solver  # noqa: F401
from .api import bundle_adjust, bundle_adjustment, serialize_params, deserialize_params  # noqa: F401
from . import calibration  # noqa: F401
from .triangulation import triangulate  # noqa: F401
from . import geometry  # noqa: F401
from .geometry import (project_points, project_to_cameras, apply_rigid_transform, keypoint_reprojection_errors, refine_triangulation, triangulate_consensus, refine_extrinsics, ExtrinsicsRefinement, rigid_transform_from_correspondences,  # noqa: F401
                       estimate_relative_pose, extrinsics_from_keypoints, KeypointExtrinsics, draw_samples, refine_cameras, CameraRefinement,
                       resect_camera, resect_cameras, CameraResection, draw_resection_samples,
                       rodrigues, rodrigues_inv, get_transformation_matrix, get_transformation_vector, get_projection_matrix, euclidean_to_homogenous, homogeneous_to_euclidean)
from .io import save_calibration, load_calibration  # noqa: F401
from .diagnostics import reprojection_errors, undistort_points  # noqa: F401
from .flatibration import get_floor_points, flatibrate, center_arena, flip_z_axis  # noqa: F401
from .detection import detect_chessboard, detect_chessboards, reorder_chessboard_corners, generate_chessboard_objpoints, extend_grid, summarize_detections  # noqa: F401
from .uncertainty import calibration_uncertainty, CalibrationUncertainty, triangulation_uncertainty, TriangulationUncertainty  # noqa: F401
from . import trajectory  # noqa: F401
from .trajectory import smooth_trajectories, TrajectorySmoothing, trajectory_uncertainty, TrajectoryUncertainty  # noqa: F401
from .trajectory import estimate_accel_std, trajectory_evidence, AccelEstimate, TrajectoryEvidence  # noqa: F401
from .trajectory import refine_trajectories, refine_trajectories_system, TrajectoryRefinement, TrajectoryRefinementSystem, TRAJECTORY_REFINE_STATUS  # noqa: F401
from . import skeleton  # noqa: F401
from .skeleton import refine_skeleton, refine_skeleton_system, estimate_bone_lengths, SkeletonRefinement, SkeletonSystem, BoneLengths  # noqa: F401
from .skeleton import refine_skeleton_trajectories, refine_skeleton_trajectories_system, SkeletonTrajectoryRefinement, SkeletonTrajectorySystem  # noqa: F401
from .calibration import calibrate, get_intrinsics, estimate_pose, estimate_all_extrinsics, consensus_calib_poses, get_camera_spanning_tree, estimate_pairwise_camera_transform  # noqa: F401

__all__ = ["bundle_adjust", "bundle_adjustment", "serialize_params", "deserialize_params", "ops", "solver", "synth", "calibration", "calibrate", "triangulate", "get_intrinsics",
           "save_calibration", "load_calibration", "reprojection_errors", "undistort_points", "estimate_pose", "estimate_all_extrinsics", "consensus_calib_poses", "get_camera_spanning_tree", "estimate_pairwise_camera_transform",
           "get_floor_points", "flatibrate", "center_arena", "flip_z_axis",
           "detect_chessboard", "detect_chessboards", "reorder_chessboard_corners", "generate_chessboard_objpoints", "extend_grid", "summarize_detections",
           "geometry", "project_points", "project_to_cameras", "apply_rigid_transform", "keypoint_reprojection_errors", "refine_triangulation", "triangulate_consensus", "refine_extrinsics", "ExtrinsicsRefinement", "rigid_transform_from_correspondences",
           "estimate_relative_pose", "extrinsics_from_keypoints", "KeypointExtrinsics", "draw_samples", "refine_cameras", "CameraRefinement",
           "resect_camera", "resect_cameras", "CameraResection", "draw_resection_samples",
           "rodrigues", "rodrigues_inv", "get_transformation_matrix", "get_transformation_vector", "get_projection_matrix", "euclidean_to_homogenous", "homogeneous_to_euclidean",
           "calibration_uncertainty", "CalibrationUncertainty", "triangulation_uncertainty", "TriangulationUncertainty",
           "trajectory", "smooth_trajectories", "TrajectorySmoothing", "trajectory_uncertainty", "TrajectoryUncertainty",
           "estimate_accel_std", "trajectory_evidence", "AccelEstimate", "TrajectoryEvidence",
           "refine_trajectories", "refine_trajectories_system", "TrajectoryRefinement", "TrajectoryRefinementSystem", "TRAJECTORY_REFINE_STATUS",
           "skeleton", "refine_skeleton", "refine_skeleton_system", "estimate_bone_lengths", "SkeletonRefinement", "SkeletonSystem", "BoneLengths",
           "refine_skeleton_trajectories", "refine_skeleton_trajectories_system", "SkeletonTrajectoryRefinement", "SkeletonTrajectorySystem"]
