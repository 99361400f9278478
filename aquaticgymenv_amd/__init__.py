"""aquaticgymenv_amd: the batched aquatic-navigation environment and its training stack in HIP for gfx950.  The classes live
in their modules (batched, qpolicy, qbank, learner, ...), each of which loads its own library when it is first used; importing
the package itself loads none, so that `aquaticgymenv_amd.build` works before anything is compiled."""

__all__ = ["EvolutionStrategy"]


def __getattr__(name):
    if name == "EvolutionStrategy":
        from .evolution import EvolutionStrategy
        return EvolutionStrategy
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
