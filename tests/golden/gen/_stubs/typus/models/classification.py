"""typus.models.classification: the two result records as dataclasses with the fields postprocessing.py reads and writes."""
from dataclasses import dataclass, field
from typing import Any, List, Optional, Tuple

from typus.constants import RankLevel


@dataclass
class TaskPrediction:
    rank_level: RankLevel
    temperature: float
    predictions: List[Tuple[int, float]] = field(default_factory=list)


@dataclass
class HierarchicalClassificationResult:
    taxonomy_context: Any
    tasks: List[TaskPrediction]
    subtree_roots: Optional[Any] = None
