"""MI355X-native drop-in for the reference package `image_diffusion` (sampling hot path only).

Same module / symbol names as `amortised diffusion/image_diffusion/` for the path SURVEY.md section 8
scopes: nn, unet, sde_diffusion, conditioning, likelihoods, sampling, and loss_functions as a forward-only value (no autograd graph).
bound (the variational bound in bits/dim) has no reference counterpart.  Training, logging, datasets and plotting modules of the
reference are out of scope and not provided.
"""
from . import bound, conditioning, likelihoods, loss_functions, nn, sampling, sde_diffusion, unet  # noqa: F401
