"""Batched tiled prediction: the notebook loop of the reference (notebooks/EvaluateJointIndi.ipynb cells 23-26: one tile
per ``test()`` call, 490 strictly serial calls, numpy stitch on the host) as a device-resident pipeline: gather tiles on
the GPU -> batches of tiles through the sampler -> (multi-GPU: one all-gather) -> HIP stitch into the (N,H,W,C) canvas.
Every driver is importable from here; they live in three siblings: ``tile_predict`` (every tile runs its own chain; what
all drivers share), ``frame_predict`` (every frame is one state) and ``mixed_predict`` (the mixed-input evaluation)."""
from .frame_predict import frame_sample, fused_sample, input_frames, predict_stack_frames  # noqa: F401
from .mixed_predict import (REFINE_SCOPES, choose_times, evaluate_time_predictor, gather_pred_t,  # noqa: F401
                            predict_tiled_mixed, predict_tiled_refined)
from .tile_predict import TileExchange, _batches, predict_stack, predict_tiled, sample_tiles, store_kept  # noqa: F401
