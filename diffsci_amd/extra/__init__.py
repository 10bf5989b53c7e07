"""Tools around the models (reference: diffsci/extra).  Built: the chunked volume decode, and the two generators of large latent
volumes it decodes -- a grid of cubes inpainted against their neighbours, and blocks extended along the last axis."""
from .chunk_decode import Tile, chunk_decode_strategy_b_3d, decode_plan, stage_radii_and_scales  # noqa: F401
from .fillinginpainting import Cube, grid_plan, sample_grid_volume  # noqa: F401
from .sequentialinpainting import sample_sequential_z  # noqa: F401
