"""Stand-in for the `typus` package: only the names linnaeus/inference/postprocessing.py imports (fixture generation only)."""
