"""Baseline codecs the paper measures ESC against, on the same native path: `from esc.baselines import DAC, DACFile`, and the losses the DAC
baseline trains against: `from esc.baselines import L1Loss, SISDRLoss, MultiScaleSTFTLoss, MelSpectrogramLoss` (esc.baselines.loss)."""
from . import loss  # noqa: F401
from .dac import DAC, DACFile  # noqa: F401
from .loss import L1Loss, MelSpectrogramLoss, MultiScaleSTFTLoss, SISDRLoss  # noqa: F401

__all__ = ["DAC", "DACFile", "L1Loss", "SISDRLoss", "MultiScaleSTFTLoss", "MelSpectrogramLoss", "loss"]
