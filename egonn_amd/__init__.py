"""egonn_amd — MI355X-native descriptor-extraction path of EgoNN (reference: jac99/Egonn).

Public surface mirrors the reference: ModelParams (misc/utils.py), model_factory (models/model_factory.py),
CartesianQuantizer / PolarQuantizer (datasets/quantization.py), plus DescriptorExtractor (the
compute_embedding slice of eval/evaluate.py).  All arithmetic runs in libegonn_hip.so (hand-written HIP for
gfx950, C ABI in include/egonn_hip.h); importing the package does not need a GPU, using it does.
"""
from .params import ModelParams
from .quantization import CartesianQuantizer, PolarQuantizer, Quantizer
from .model import MinkGL, MinkHead, MinkTrunk, model_factory, create_egonn_model
from .minkloc import MinkFPN, MinkLoc, MinkLoc3D
from .evaluator import DescriptorExtractor, GraphExtractor, GlobalExtractor, GlobalGraphExtractor
from .rotations import evaluate_with_rotations
from .stream import StreamingExtractor
from .local_loss import (KeypointLoss, CorrespondenceLoss, KeypointCorrLoss, make_local_loss, BatchedKeypointCorrLoss,
                         local_loss_packed)
from .train import EgoNNTrainStep
from .registration import (get_ransac_result, calculate_repeatability, register_pairs, evaluate_local, match_mutual,
                           RegistrationResult, voxel_downsample, icp_pairs, refine_pairs, icp, estimate_normals,
                           icp_point_to_plane, spectral_verify)
from .augment import (TrainTransform, TrainSetTransform, TrainBatcher, JitterPoints, RemoveRandomPoints, RandomTranslation,
                      RandomRotation, RemoveRandomBlock, RandomFlip, RigidPerturbation, AugmentParams, augment_points)
from .tuples import (TrainingTuple, EvaluationTuple, EvaluationSet, save_training_tuples, load_training_tuples, radius_neighbors,
                     count_within, relative_poses, CloudBank, generate_training_tuples, filter_query_elements,
                     generate_evaluation_set, TupleIndex, BatchSampler, TrainingSet)
from .relocalize import KeypointMap, verify_candidates, Relocalizer, evaluate_relocalization
from .loop_closure import knn_window, time_windows, detect_loops, LoopDetector, evaluate_loop_closure
from .pose_graph import (pose_graph_cost, pose_graph_hessvec, optimize_pose_graph, odometry_edges, loop_edges,
                         optimize_trajectory)
from .loop_consistency import filter_loops, loop_cycle_errors
from .mapping import VoxelMap, build_map, refine_against_map, NDTMap, build_ndt_map
from .scan_context import ScanContext, ScanContextManager, sc2rk, distance_sc, evaluate as evaluate_scan_context

__all__ = ["ModelParams", "model_factory", "create_egonn_model", "MinkGL", "MinkHead", "MinkTrunk",
           "CartesianQuantizer", "PolarQuantizer", "Quantizer", "DescriptorExtractor", "GraphExtractor", "GlobalExtractor", "GlobalGraphExtractor",
           "evaluate_with_rotations", "StreamingExtractor", "MinkFPN", "MinkLoc", "MinkLoc3D",
           "KeypointLoss", "CorrespondenceLoss", "KeypointCorrLoss", "make_local_loss",
           "BatchedKeypointCorrLoss", "local_loss_packed", "EgoNNTrainStep",
           "get_ransac_result", "calculate_repeatability", "register_pairs", "evaluate_local", "match_mutual", "RegistrationResult",
           "voxel_downsample", "icp_pairs", "refine_pairs", "icp", "estimate_normals", "icp_point_to_plane", "spectral_verify",
           "TrainTransform", "TrainSetTransform", "TrainBatcher", "JitterPoints", "RemoveRandomPoints", "RandomTranslation",
           "RandomRotation", "RemoveRandomBlock", "RandomFlip", "RigidPerturbation", "AugmentParams", "augment_points",
           "TrainingTuple", "EvaluationTuple", "EvaluationSet", "save_training_tuples", "load_training_tuples", "radius_neighbors",
           "count_within", "relative_poses", "CloudBank", "generate_training_tuples", "filter_query_elements",
           "generate_evaluation_set", "TupleIndex", "BatchSampler", "TrainingSet",
           "KeypointMap", "verify_candidates", "Relocalizer", "evaluate_relocalization",
           "knn_window", "time_windows", "detect_loops", "LoopDetector", "evaluate_loop_closure",
           "pose_graph_cost", "pose_graph_hessvec", "optimize_pose_graph", "odometry_edges", "loop_edges", "optimize_trajectory",
           "filter_loops", "loop_cycle_errors", "VoxelMap", "build_map", "refine_against_map", "NDTMap", "build_ndt_map",
           "ScanContext", "ScanContextManager", "sc2rk", "distance_sc", "evaluate_scan_context"]
