"""A/B helpers for the micro-benchmarks: bind another build of libleco_hip (same C ABI) and time launch chains from ONE
hipGraph.  `leco_amd.graphs` declares the graph entry points on whichever library object is bound."""
import os

from leco_amd import graphs, hip


def use_lib(path: str) -> None:
    os.environ["LECO_HIP_LIB"] = path          # (hip.is_emulated(): a side build named here is a GPU library)
    hip._use_library(path)


def graph_us(chain, reps=20):
    """us per op of `chain` (a list of ops.Op) replayed from one captured graph"""
    return graphs.replay_us(chain, reps) / len(chain)
