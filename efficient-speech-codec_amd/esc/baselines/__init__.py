"""Baseline codecs the paper measures ESC against, on the same native path: `from esc.baselines import DAC`."""
from .dac import DAC  # noqa: F401

__all__ = ["DAC"]
