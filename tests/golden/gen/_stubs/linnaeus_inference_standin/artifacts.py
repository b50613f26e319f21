"""The two names postprocessing.py imports from .artifacts; it uses them as annotations only."""


class ClassIndexMapData:
    pass


class TaxonomyData:
    pass
