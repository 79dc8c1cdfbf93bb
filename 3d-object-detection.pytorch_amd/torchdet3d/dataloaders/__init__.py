from .gpu_crops import FrameCropper, crop_cords_from_keypoints
from .objectron import Objectron, AugmentPipeline, build_augmentations, collate_crops
from .gpu_loader import GpuAugmentLoader
