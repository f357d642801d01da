from .attribution import feature_scores, grad_times_act
from .cache import Cache, FeatureCache, FeatureImageCache, generate_split_indices
from .loader import FeatureDataset, FeatureRecords, sample_example_records, split_path, top_example_records
from .stats import FeatureStats, cos, get_neighbors, logits
from .coact import CoactStats, coact_neighbors
from .recon import ReconStats
from .hist import ActHist
from .pos import PosProfile
from .tokens import TokenProfile
from .edits import FeatureEdits, RowEdits
from .hooks import attribution_sae_hook, clamp_features_max, clamp_features_rows, sae_reconstruct, transcoder_hook
from .patching import Attribution

__all__ = ["Cache", "FeatureCache", "FeatureImageCache", "generate_split_indices",
           "clamp_features_max", "attribution_sae_hook", "sae_reconstruct", "grad_times_act", "feature_scores", "FeatureDataset", "FeatureRecords", "split_path", "Attribution",
           "FeatureStats", "FeatureEdits", "RowEdits", "clamp_features_rows", "top_example_records", "sample_example_records", "cos", "get_neighbors", "logits",
           "CoactStats", "coact_neighbors", "ReconStats", "ActHist", "PosProfile", "TokenProfile", "transcoder_hook"]
