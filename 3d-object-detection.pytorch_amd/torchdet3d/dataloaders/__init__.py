from .gpu_crops import FrameCropper, crop_cords_from_keypoints
from .objectron import Objectron, AugmentPipeline, build_augmentations, collate_crops
from .gpu_loader import GpuAugmentLoader
from .detection import ObjectronFrames, DetectionAugmentPipeline, collate_frames
from .gpu_detection_loader import GpuDetectionLoader
from .jpeg import (JpegIndex, decode_jpeg_batch, index_jpeg, collate_jpeg, plan_roi, decode_jpeg_rois, read_jpeg_header,
                   index_jpeg_device, decode_jpeg_frames)
from .detection_arena import DetectionArena, ArenaDetectionLoader, plan_arena_batch, detect_draw_host, detect_roi_plan_host
