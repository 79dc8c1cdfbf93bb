from .detection import DetectorHeadTrainer, DetectorTrainer
from .train import Trainer
