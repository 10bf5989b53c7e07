"""Autoencoder wrappers a latent KarrasModule is given (reference: diffsci/models/nets/autoencoders.py)."""
import torch


class LDMAutoencoderKLWrapper(torch.nn.Module):
    """autoencoders.py:111-146 around this package's AutoencoderKL: decode(z, has_batch_dim) is the HIP decoder; encode passes
    the AutoencoderKL's refusal through (the encoder is outside the sampling path)."""

    def __init__(self, vae):
        super().__init__()
        self.vae = vae
        self.inference = False

    def forward(self, x, has_batch_dim=True):
        return self.decode(self.encode(x, has_batch_dim), has_batch_dim)

    def encode(self, x, has_batch_dim=True, mode=False):
        if not has_batch_dim:
            x = x.unsqueeze(0)
        res = self.vae.encode(x)
        res = res.mode() if mode else res.sample()
        if not has_batch_dim:
            res = res[0]
        return res

    def decode(self, z, has_batch_dim=True):
        if not has_batch_dim:
            z = z.unsqueeze(0)
        res = self.vae.decode(z)
        if not has_batch_dim:
            res = res[0]
        return res
