"""A package to load linnaeus/inference/postprocessing.py into by file path: the real linnaeus.inference imports its whole serving
stack on import.  postprocessing.py's `from .artifacts import ...` resolves to the module beside this file."""
