from .prediction import Prediction, PredictionBatch
from .monster_diffusion import MonsterDiffusion
