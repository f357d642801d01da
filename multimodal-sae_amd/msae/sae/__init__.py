from .config import SaeConfig, TrainConfig
from .probe import ProbeOutput
from .sae import EncoderOutput, ForwardOutput, ReconOutput, Sae

__all__ = ["Sae", "SaeConfig", "TrainConfig", "EncoderOutput", "ForwardOutput", "ProbeOutput", "ReconOutput"]
