"""Earlier import path of the fused-PPA gate; everything lives in ppa_plan."""
from .ppa_plan import *  # noqa: F401,F403
