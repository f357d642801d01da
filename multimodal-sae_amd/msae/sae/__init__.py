from .config import SaeConfig, TrainConfig
from .probe import ProbeOutput
from .sae import BatchForwardOutput, EncoderOutput, ForwardOutput, JumpForwardOutput, ReconOutput, RefitOutput, Sae

__all__ = ["Sae", "SaeConfig", "TrainConfig", "EncoderOutput", "ForwardOutput", "BatchForwardOutput", "JumpForwardOutput", "ProbeOutput", "ReconOutput", "RefitOutput"]
