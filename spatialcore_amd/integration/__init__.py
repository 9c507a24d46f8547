"""spatialcore_amd.integration -- what comes between pca and neighbors on more than one sample: Harmony batch correction
of the embedding (sc_harmony_*)."""
from spatialcore_amd.integration.harmony import harmony_integrate

__all__ = ["harmony_integrate"]
