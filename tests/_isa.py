"""tools/isa_listing.py for the CPU tests: the device listing of a library is compiled once and shared (read-only) by the
tests that look at it."""
import functools
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def module():
    spec = importlib.util.spec_from_file_location("isa_listing", os.path.join(ROOT, "tools", "isa_listing.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def listing(name):
    """-> isa_listing.listing() of library `name` (policy, learner, episodes)"""
    return module().listing(name)


@functools.lru_cache(maxsize=None)
def kernels(name):
    """-> isa_listing.kernels() of that listing"""
    return module().kernels(listing(name))
