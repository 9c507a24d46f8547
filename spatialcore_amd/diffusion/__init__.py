"""MI355X-native ``spatialcore.diffusion`` (the last module the reference's roadmap names: "Diffusion maps, pseudotime
analysis"): the diffusion map of Haghverdi et al. 2016 on a locally scaled Gaussian kernel over exact nearest neighbours
in feature space, and diffusion pseudotime from a root cell on the stored map."""

from spatialcore_amd.diffusion.maps import diffusion_map, diffusion_pseudotime

__all__ = ["diffusion_map", "diffusion_pseudotime"]
