"""``data/LRHR_dataset.py`` of the reference for the SR3 configurations, with its items made on the device.

``datatype='img'`` (:28-40, :88-99) reads the PNG folders ``lr_{l}/``, ``hr_{r}/`` and ``sr_{l}_{r}/`` that
``prepare_data.py`` writes; ``datatype='lmdb'`` raises ``DsxError`` (lmdb is not a dependency).  One addition:
``datatype='hr_only'`` takes a folder of source images and makes LR and SR on the device with
``prepare_data.resize_multiple``, so ``prepare_data`` need not be run first.

Items are ``{'HR', 'SR', 'Index'}`` (+ ``'LR'`` with ``need_LR``), fp32 CHW device tensors in (-1, 1).  As a superset
for the reference's rot they also carry ``'input'`` (= SR) and ``'target'`` (= HR): the reference's own ``DDPM.test``
reads ``data['input']``, which its dataset never supplies.  ``batch(indices)`` gives the stacked device batch in one
pass.  Items live on the GPU, so a DataLoader over this dataset must not use worker processes
(``data.create_dataloader`` sets ``num_workers=0``).
"""
import numpy as np
import torch
from torch.utils.data import Dataset

from .._lib import DsxError
from . import util as Util


class LRHRDataset(Dataset):
    def __init__(self, dataroot, datatype, l_resolution=16, r_resolution=128, split='train', data_len=-1, need_LR=False,
                 resample=None):
        self.datatype = datatype
        self.l_res = l_resolution
        self.r_res = r_resolution
        self.data_len = data_len if data_len is not None else -1
        self.need_LR = need_LR
        self.split = split
        self.resample = resample

        if datatype == 'lmdb':
            raise DsxError("LRHRDataset(datatype='lmdb'): lmdb is out of scope (not a dependency); write PNG folders "
                           "with data/prepare_data.py and use datatype='img', or datatype='hr_only' on the source images")
        elif datatype == 'img':
            self.sr_path = Util.get_paths_from_images('{}/sr_{}_{}'.format(dataroot, l_resolution, r_resolution))
            self.hr_path = Util.get_paths_from_images('{}/hr_{}'.format(dataroot, r_resolution))
            if self.need_LR:
                self.lr_path = Util.get_paths_from_images('{}/lr_{}'.format(dataroot, l_resolution))
        elif datatype == 'hr_only':
            self.hr_path = Util.get_paths_from_images('{}'.format(dataroot))
        else:
            raise NotImplementedError('data_type [{:s}] is not recognized.'.format(str(datatype)))
        self.dataset_len = len(self.hr_path)
        if self.data_len <= 0:
            self.data_len = self.dataset_len
        else:
            self.data_len = min(self.data_len, self.dataset_len)

    def __len__(self):
        return self.data_len

    @staticmethod
    def _read(path):
        from PIL import Image
        return np.array(Image.open(path).convert("RGB"))

    def _u8(self, indices):
        """-> uint8 device batches {'LR' (with need_LR), 'SR', 'HR'}, each (B, size, size, 3), in index order."""
        stack = lambda paths: Util.to_device_u8(torch.from_numpy(np.stack([self._read(paths[i]) for i in indices])))
        if self.datatype == 'img':
            out = {'SR': stack(self.sr_path), 'HR': stack(self.hr_path)}
            if self.need_LR:
                out['LR'] = stack(self.lr_path)
            return out
        from . import prepare_data as P
        resample = P.BICUBIC if self.resample is None else self.resample
        src = [self._read(self.hr_path[i]) for i in indices]
        out = {k: [None] * len(src) for k in ('LR', 'HR', 'SR')}
        by_shape = {}
        for k, a in enumerate(src):
            by_shape.setdefault(a.shape, []).append(k)
        for ks in by_shape.values():               # one batched resize per source size
            t = Util.to_device_u8(torch.from_numpy(np.stack([src[k] for k in ks])))
            for name, res in zip(('LR', 'HR', 'SR'), P.resize_multiple(t, (self.l_res, self.r_res), resample)):
                for j, k in enumerate(ks):
                    out[name][k] = res[j]
        keys = ('LR', 'HR', 'SR') if self.need_LR else ('HR', 'SR')
        return {k: torch.stack(out[k]) for k in keys}

    def batch(self, indices):
        """The items of ``indices`` stacked: (B, 3, size, size) fp32 device tensors and an int64 'Index'."""
        indices = [int(i) for i in indices]
        if self.split == 'train':
            Util.transform_augment([], split='train')           # raises: training augmentation is out of scope
        u8 = self._u8(indices)
        out = {k: Util.u8_to_tensor(v, (-1, 1)) for k, v in u8.items()}
        out['Index'] = torch.tensor(indices, dtype=torch.int64)
        out['input'], out['target'] = out['SR'], out['HR']
        return out

    def __getitem__(self, index):
        b = self.batch([index])
        item = {k: v[0] for k, v in b.items() if k not in ('Index', 'input', 'target')}
        item['Index'] = index
        item['input'], item['target'] = item['SR'], item['HR']
        return item
