#!/usr/bin/env python3
"""``infer.py`` — the reference's SR3 inference entry point (infer.py:13-100 and its flags) on MI355X, from image files
to written PNGs and PSNR / SSIM:

    python -m diffsplitting_amd.infer -c config/sr_sr3_16_128.json -p val -gpu 0 --dataroot <folder>

The config is consumed unchanged.  ``datasets.val`` names the image folders (``datatype: "img"``: the ``lr_*/hr_*/sr_*``
PNG folders of data/prepare_data.py; ``"hr_only"``: a folder of source images, resized on the device).  Beyond the
reference's flags: ``--dataroot`` overrides ``datasets.val.dataroot``, ``--batch`` images go through the sampler at once
(the reference's loader yields one), ``--steps`` overrides ``beta_schedule.val.n_timestep``, ``--dtype`` the MFMA
operand type and ``--seed`` torch's generator, from which the device noise is seeded.  ``--sample-seed S`` draws every
image's noise from its own stream instead (seed S, sample id = the image's ordinal in the validation set): image 37 is
the same whatever ``--batch`` it ran in and whichever images ran before it.  ``--solver {ddim,dpmpp2m} --solver-steps K
[--eta E] [--spacing uniform|logsnr]`` samples with a few-step solver over K timesteps of the schedule the checkpoint
was trained on (``model/solvers.py``; refused by name for a sampler that is not Gaussian); without ``--solver`` the run is
the ancestral loop as before.

Per image the run writes ``{step}_{idx}_hr.png`` (ground truth), ``{step}_{idx}_inf.png`` (the upsampled input the
model is conditioned on, the reference's 'INF' visual) and ``{step}_{idx}_sr.png`` (the sample) into ``path.results``
through ``core.metrics.tensor2img`` / ``save_img``, and logs the mean PSNR and SSIM of sample against ground truth
(the reference's split.py:312-313), taken for the whole batch by ``core.metrics.image_metrics``.
"""
import argparse
import logging
import os

import numpy as np
import torch

from . import data as Data
from .core import logger as Logger
from .core import metrics as Metrics
from .model import create_model


def _save(t, path):
    """One (3, H, W) tensor in (-1, 1) -> PNG: tensor2img gives HWC, save_img takes channel-first."""
    Metrics.save_img(np.transpose(Metrics.tensor2img(t), (2, 0, 1)), path)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('-c', '--config', type=str, default='config/sr_sr3_64_512.json', help='JSON file for configuration')
    ap.add_argument('-p', '--phase', type=str, choices=['val'], help='val(generation)', default='val')
    ap.add_argument('-gpu', '--gpu_ids', type=str, default=None)
    ap.add_argument('-debug', '-d', action='store_true')
    ap.add_argument('-enable_wandb', action='store_true')
    ap.add_argument('-log_infer', action='store_true')
    ap.add_argument('-rootdir', type=str, default='.')
    ap.add_argument('--dataroot', type=str, default=None, help='override datasets.val.dataroot')
    ap.add_argument('--batch', type=int, default=16, help='images per sampler call')
    ap.add_argument('--steps', type=int, default=None, help='override beta_schedule.val.n_timestep')
    ap.add_argument('--dtype', type=str, default=None, choices=['f32', 'bf16', 'f16'])
    ap.add_argument('--seed', type=int, default=None)
    ap.add_argument('--sample-seed', type=int, default=None,
                    help='per-sample noise streams: image k of the validation set draws from the stream (seed, k)')
    ap.add_argument('--solver', type=str, default=None, choices=['ddim', 'dpmpp2m'],
                    help='few-step sampling over --solver-steps timesteps of the trained schedule')
    ap.add_argument('--solver-steps', type=int, default=None)
    ap.add_argument('--eta', type=float, default=0.0, help='ddim only: 0 deterministic .. 1 ancestral variance')
    ap.add_argument('--spacing', type=str, default=None, choices=['uniform', 'logsnr'])
    args = ap.parse_args(argv)
    if args.batch < 1:
        raise SystemExit('--batch must be >= 1')
    if args.solver is None and (args.solver_steps is not None or args.eta != 0.0 or args.spacing is not None):
        raise SystemExit('--solver-steps, --eta and --spacing belong to --solver')
    if args.solver is not None and args.solver_steps is None:
        raise SystemExit('--solver needs --solver-steps')
    opt = Logger.parse(args)
    logging.basicConfig(level=logging.INFO, format='%(asctime)s %(message)s')
    log = logging.getLogger('base')
    if args.dtype:
        opt['model']['compute_dtype'] = args.dtype
    if args.steps:
        opt['model']['beta_schedule']['val']['n_timestep'] = args.steps
    if opt['gpu_ids'] is None:
        opt['gpu_ids'] = [0]                                  # the engine runs on the device only
    torch.cuda.set_device(opt['gpu_ids'][0])
    if args.seed is not None:
        torch.manual_seed(args.seed)

    # dataset
    val_set = val_loader = None
    for phase, dataset_opt in (opt['datasets'] or {}).items():
        if phase == 'val':
            if args.dataroot:
                dataset_opt['dataroot'] = args.dataroot
            val_set = Data.create_dataset(dataset_opt, phase)
            val_loader = Data.create_dataloader(val_set, dataset_opt, phase)
    if val_set is None:
        raise SystemExit('the config has no datasets.val section')
    log.info('Initial Dataset Finished')

    # model
    diffusion = create_model(opt)
    log.info('Initial Model Finished')
    diffusion.set_new_noise_schedule(opt['model']['beta_schedule']['val'], schedule_phase='val')
    if args.solver is not None:                               # refused by name for a sampler that is not Gaussian
        diffusion.set_solver(args.solver, steps=args.solver_steps, eta=args.eta, spacing=args.spacing)

    log.info('Begin Model Inference.')
    current_step = 0
    idx = 0
    result_path = '{}'.format(opt['path']['results'])
    os.makedirs(result_path, exist_ok=True)
    if args.batch == 1:
        batches = val_loader
    else:
        batches = (val_set.batch(range(i, min(i + args.batch, len(val_set)))) for i in range(0, len(val_set), args.batch))
    psnrs, ssims, files = [], [], []
    for val_data in batches:
        diffusion.feed_data(val_data)
        if args.sample_seed is None:
            diffusion.test(continuous=False)
        else:                                                 # idx: images done so far = this batch's first ordinal
            n_batch = int(diffusion.data['HR'].shape[0])
            diffusion.test(continuous=False, seed=args.sample_seed, sample_ids=range(idx, idx + n_batch))
        sample = diffusion.netG.last_full_batch               # test() returns the last image only (ret_img[-1])
        hr, inf = diffusion.data['HR'], diffusion.data['SR']
        psnr, ssim = Metrics.image_metrics(sample, hr, min_max=(-1, 1))
        psnrs += psnr.tolist()
        ssims += ssim.tolist()
        for b in range(sample.shape[0]):
            idx += 1
            stem = '{}/{}_{}'.format(result_path, current_step, idx)
            _save(hr[b], stem + '_hr.png')
            _save(sample[b], stem + '_sr.png')
            _save(inf[b], stem + '_inf.png')
            files.append(stem)
    avg_psnr, avg_ssim = float(np.mean(psnrs)), float(np.mean(ssims))
    log.info('# Validation # PSNR: {:.4e}'.format(avg_psnr))
    log.info('# Validation # SSIM: {:.4e}'.format(avg_ssim))
    return {'psnr': avg_psnr, 'ssim': avg_ssim, 'per_image_psnr': psnrs, 'per_image_ssim': ssims, 'files': files,
            'diffusion': diffusion}


if __name__ == '__main__':
    main()
