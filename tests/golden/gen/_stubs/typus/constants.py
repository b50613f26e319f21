"""typus.constants.RankLevel as a plain Enum: postprocessing.py reads only `.value` and `.name`."""
from enum import Enum


class RankLevel(Enum):
    L10 = 10
    L20 = 20
    L30 = 30
    L40 = 40
    L50 = 50
    L60 = 60
    L70 = 70
