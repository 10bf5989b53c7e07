"""Tools around the models (reference: diffsci/extra).  Built: the chunked volume decode, and the two generators of large latent
volumes it decodes -- a grid of cubes inpainted against their neighbours, and blocks extended along the last axis; and the
post-training periodization of a network along chosen axes (punetg_converters), and periodization around any network by
expanding, cropping and blending (periodizer)."""
from .chunk_decode import Tile, chunk_decode_strategy_b_3d, decode_plan, stage_radii_and_scales  # noqa: F401
from .fillinginpainting import Cube, grid_plan, sample_grid_volume  # noqa: F401
from .sequentialinpainting import sample_sequential_z  # noqa: F401
from .punetg_converters import convert_conv_to_circular, count_conv_layers  # noqa: F401
from .periodizer import DiffusionPeriodizer, PeriodicSamplerWrapper, measure_periodicity_error  # noqa: F401
