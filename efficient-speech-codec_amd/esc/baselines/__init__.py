"""Baseline codecs the paper measures ESC against, on the same native path: `from esc.baselines import DAC, DACFile`, and the losses the DAC
baseline trains against: `from esc.baselines import L1Loss, SISDRLoss, MultiScaleSTFTLoss, MelSpectrogramLoss, GANLoss` (esc.baselines.loss).
`Discriminator` is esc.models.Discriminator, the class the reference defines twice (`dac.model.Discriminator`)."""
from . import loss  # noqa: F401
from ..models.discriminator import Discriminator  # noqa: F401
from .dac import DAC, DACFile  # noqa: F401
from .loss import GANLoss, L1Loss, MelSpectrogramLoss, MultiScaleSTFTLoss, SISDRLoss  # noqa: F401

__all__ = ["DAC", "DACFile", "Discriminator", "L1Loss", "SISDRLoss", "MultiScaleSTFTLoss", "MelSpectrogramLoss", "GANLoss", "loss"]
