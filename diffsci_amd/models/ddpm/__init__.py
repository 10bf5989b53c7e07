"""The discrete DDPM / DDIM sampler family (reference: diffsci/models/ddpm).  Only v2 is built -- the reference star-exports it as
``diffsci.models.ddpmv2``; v1 is its older duplicate."""
from . import v2 as ddpmv2  # noqa: F401
