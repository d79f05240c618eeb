"""gdl -- MI355X-native DGL audio-visual training step (host side over libgdl_hip.so).

Nothing here computes on the CPU: every operator is a hand-written gfx950 kernel behind the
C ABI of include/gdl_hip.h, and importing a compute entry point without the built library
raises.
"""
from . import _lib  # noqa: F401
from ._lib import GdlError  # noqa: F401


def __getattr__(name):
    """`gdl.DGLTrainer` / `gdl.UnimodalTrainer`: the two runners, and `gdl.feature_diversity`, main.py's per-step monitor on a
    feature map, and `gdl.journal`, the step journal's module (`gdl.journal.COLUMNS`), and the device-side waveform staging of
    gdl.data (`gdl.stage_audio`, `gdl.wave_log_spectrogram`, `gdl.wave_descriptors`, `gdl.pack_clips`, `gdl.wave_limit`,
    `gdl.random_wave_starts`, `gdl.AUDIO_STAGES`), and the linear probe of gdl.probe (`gdl.extract_features`, `gdl.FeatureBank`,
    `gdl.LinearProbe`, `gdl.probe_order`, `gdl.multistep_lr`), and `gdl.ScoreBank`, the evaluation report of gdl.evaluate (mAP,
    top-k, confusion), and the class prototypes of gdl.prototypes (`gdl.Prototypes`, `gdl.prototype_logits`: prototypical modal
    rebalance on the joint step), and `gdl.MLATrainer` with its schedule helper `gdl.mla_alpha` (gdl.mla: alternating unimodal
    training on a shared head), and the device-resident epoch loader of gdl.loader (`gdl.DeviceDataset`, `gdl.DeviceLoader`: the
    shuffle, the window starts, the crop boxes and the flips planned on the device) -- imported on first use (they import torch)."""
    if name in ("DeviceDataset", "DeviceLoader"):
        from . import loader

        return getattr(loader, name)
    if name in ("MLATrainer", "mla_alpha"):
        from . import mla

        return getattr(mla, name)
    if name in ("Prototypes", "prototype_logits"):
        from . import prototypes

        return getattr(prototypes, name)
    if name == "ScoreBank":
        from .evaluate import ScoreBank

        return ScoreBank
    if name in ("stage_audio", "wave_log_spectrogram", "wave_descriptors", "pack_clips", "wave_limit", "random_wave_starts", "AUDIO_STAGES"):
        from . import data

        return getattr(data, name)
    if name in ("extract_features", "FeatureBank", "LinearProbe", "probe_order", "multistep_lr"):
        from . import probe

        return getattr(probe, name)
    if name == "journal":
        import importlib

        return importlib.import_module(".journal", __name__)
    if name == "feature_diversity":
        from .diversity import feature_diversity

        return feature_diversity
    if name == "DGLTrainer":
        from .trainer import DGLTrainer

        return DGLTrainer
    if name == "UnimodalTrainer":
        from .unimodal import UnimodalTrainer

        return UnimodalTrainer
    raise AttributeError(f"module 'gdl' has no attribute {name!r}")
