from .detection import DetectorHeadTrainer
from .train import Trainer
