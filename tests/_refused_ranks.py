"""driver of the test_ranks_are_refused_before_any_exchange tests: the calls of one family (tests/_refused_ranks_worker.py FAMILIES) made by rank 1
alone of a two-rank context.  A refusal that had become collective would leave rank 1 waiting for rank 0 until the worker's own limit."""
import json

from _ranks import run_spec


def refused_ranks(tmp_path, family, N=40, F=4):
    """both ranks' results: {"errors": one text per call made ("" if it succeeded), "faces", "first": of the collective mesh afterwards}"""
    outs = run_spec("_refused_ranks_worker.py", tmp_path, "refused", "json", 2, 150, {"family": family, "N": N, "F": F, "callers": [1]})
    return [json.load(open(o)) for o in outs]
