"""Tools around the models (reference: diffsci/extra).  Built: the chunked volume decode."""
from .chunk_decode import Tile, chunk_decode_strategy_b_3d, decode_plan, stage_radii_and_scales  # noqa: F401
