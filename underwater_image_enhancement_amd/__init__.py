"""MI355X-native underwater image enhancement: hand-written HIP kernels (gfx950) behind the reference's API.

Importing this package does not touch the GPU; the first call into :mod:`api` loads ``lib/libuwie.so`` and
fails loudly when it (or a ROCm device) is missing -- there is no CPU fallback.
"""
from ._lib import UwieError, UwieParams, build, load  # noqa: F401
from .api import (CONFIG_QUALITY_WEIGHTS, CONFIG_STRATEGIES, DRIVER_STRATEGIES, QUALITY_KEYS, DifferentiableEnhancement, DiffEnhanceFunction, DiffEnhanceLossFunction, FEATURE_EXTRACTOR_KEYS, GatedDifferentiableEnhancement, GatedDiffEnhanceFunction, GatedDiffEnhanceLossFunction, FeatureExtractor, RefLossFunction, ReferenceLoss, PerceptualLoss, PerceptualFunction, CombinedLoss, vgg16_features16, VGGParameterNet, EnhancementPredictor, ParameterPredictor, GatedEnhancementPredictor, EndToEndTrainer, GATED_PARAM_KEYS, param_net_torch, param_net_layout, PARAM_KEYS, UnsupportedInputError, EnhancementStrategies, QualityAssessment, SixStrategies, color_correction,  # noqa: F401
                  detect_image_type, enhance, enhance_all, extract_all_features, feature_extractor_keys, feature_extractor_rows, image_tensor, process_batch, quality_scores, resize_frames,
                  select_best, training_batch, vgg_input,
                  UNDERWATER_SCORE_NAMES, UnderwaterQuality, select_best_underwater, underwater_scores,
                  REFERENCE_SCORE_NAMES, ReferenceQuality, reference_scores, select_best_reference,
                  GRAY_WORLD_STAT_NAMES, gray_world, fusion, fusion_levels)
from .classifier import StrategyClassifier  # noqa: F401
from .runtime import Device, get_device  # noqa: F401
from .streaming import StreamEnhancer  # noqa: F401

__all__ = ["enhance", "enhance_all", "fusion", "fusion_levels", "gray_world", "GRAY_WORLD_STAT_NAMES", "reference_scores", "REFERENCE_SCORE_NAMES", "ReferenceQuality", "select_best_reference", "underwater_scores", "UNDERWATER_SCORE_NAMES", "UnderwaterQuality", "select_best_underwater","process_batch", "extract_all_features", "QualityAssessment", "quality_scores", "QUALITY_KEYS", "DRIVER_STRATEGIES", "select_best", "CONFIG_STRATEGIES", "CONFIG_QUALITY_WEIGHTS", "DifferentiableEnhancement", "DiffEnhanceFunction", "GatedDifferentiableEnhancement", "GatedDiffEnhanceFunction", "ReferenceLoss", "RefLossFunction", "PerceptualLoss", "PerceptualFunction", "CombinedLoss", "vgg16_features16", "VGGParameterNet", "EnhancementPredictor", "ParameterPredictor", "GatedEnhancementPredictor", "EndToEndTrainer", "GATED_PARAM_KEYS", "param_net_torch", "param_net_layout", "PARAM_KEYS", "DiffEnhanceLossFunction", "GatedDiffEnhanceLossFunction", "FeatureExtractor", "FEATURE_EXTRACTOR_KEYS", "feature_extractor_rows", "feature_extractor_keys", "resize_frames", "image_tensor", "training_batch", "vgg_input", "SixStrategies", "EnhancementStrategies", "StrategyClassifier", "detect_image_type", "color_correction", "Device",
           "get_device", "StreamEnhancer", "UwieError", "UnsupportedInputError", "UwieParams", "build", "load"]
