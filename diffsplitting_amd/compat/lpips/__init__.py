"""``import lpips; lpips.LPIPS(net='alex')`` -> diffsplitting_amd.core.lpips.LPIPS (the notebooks' import line; weights
come from DSX_LPIPS_WEIGHTS or the constructor, never fetched)."""
from diffsplitting_amd.core.lpips import LPIPS  # noqa: F401
