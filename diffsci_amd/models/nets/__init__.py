from .punetg_config import PUNetGConfig  # noqa: F401
from .punetg import PUNetG, PUNetGCond  # noqa: F401
from .mlp import MLPCond, MLPUncond  # noqa: F401
from .adm import (ADM, ADMBaseBlock, ADMConfig, ADMDecoder, ADMDecoderBlock, ADMEncoder, ADMEncoderBlock,  # noqa: F401
                  ADMMiddleBlock, ADMTimeEmbedding)
from .embedder import PorosityEmbedder  # noqa: F401
from .dit import DiffusionTransformer  # noqa: F401
from .autoencoders import LDMAutoencoderKLWrapper  # noqa: F401
from . import autoencoderldm2d, autoencoderldm3d  # noqa: F401
# the reference star-exports both modules, the 3-D one last: these names are the volume classes
from .autoencoderldm3d import AttnBlock, AutoencoderKL, Decoder, ResnetBlock, Upsample, ddconfig  # noqa: F401
from . import vaenet  # noqa: F401
from .vaenet import VAENet, VAENetConfig  # noqa: F401
from .convit import ConVit, ConVitBlock, ConVitConfig  # noqa: F401
