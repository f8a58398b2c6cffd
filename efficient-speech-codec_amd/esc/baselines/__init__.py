"""Baseline codecs the paper measures ESC against, on the same native path: `from esc.baselines import DAC, DACFile`."""
from .dac import DAC, DACFile  # noqa: F401

__all__ = ["DAC", "DACFile"]
