"""``create_dataset`` / ``create_dataloader`` of the reference's ``data`` package (data/__init__.py:7-39) for the
validation path.  ``'train'`` is refused: the engine is inference-only.  Everything else is imported lazily, as the
reference does, so importing a submodule (``data.tiling``) pulls in nothing else."""
import logging


def create_dataloader(dataset, dataset_opt, phase):
    '''create dataloader '''
    if phase == 'val':
        import torch.utils.data
        # the items are device tensors: no worker processes (a worker must not open the GPU) and nothing to pin
        return torch.utils.data.DataLoader(dataset, batch_size=1, shuffle=False, num_workers=0, pin_memory=False)
    if phase == 'train':
        from .._lib import DsxError
        raise DsxError("create_dataloader(phase='train'): training is out of scope of the MI355X sampling engine")
    raise NotImplementedError('Dataloader [{:s}] is not found.'.format(str(phase)))


def create_dataset(dataset_opt, phase):
    '''create dataset'''
    if phase == 'train':
        from .._lib import DsxError
        raise DsxError("create_dataset(phase='train'): training is out of scope of the MI355X sampling engine")
    mode = dataset_opt['mode']
    from .LRHR_dataset import LRHRDataset as D
    dataset = D(dataroot=dataset_opt['dataroot'],
                datatype=dataset_opt['datatype'],
                l_resolution=dataset_opt['l_resolution'],
                r_resolution=dataset_opt['r_resolution'],
                split=phase,
                data_len=dataset_opt['data_len'],
                need_LR=(mode == 'LRHR')
                )
    logger = logging.getLogger('base')
    logger.info('Dataset [{:s} - {:s}] is created.'.format(dataset.__class__.__name__, str(dataset_opt['name'])))
    return dataset
