"""Where the normals of one sampling call come from.

A public sampling entry builds one ``Draws`` from the sampler's ``noise_source`` / ``noise_field`` and the call's
``seed`` / ``sample_ids``; the constructor makes every refusal before a draw is taken or a generator touched, and the
call then asks it for the initial state, for a loop's keywords or for a single step's.  Exactly one source answers:

- field:    ``noise_field(shape, draw)`` -- draw 0 is the initial state, draw ``s + 1`` the noise of step ``s``; the loop
            runs on these draws in the injected form and torch's generator is not touched;
- streams:  the per-sample noise streams ``(seed, sample_ids)`` (include/dsx.h), same ordinals, drawn on the device;
            torch's generator is not touched;
- injected: ``noise_source(shape)``, asked in the reference's draw order (parity mode, Q4); torch's generator is not
            touched (the draws must stay in order);
- default:  the device generator (``torch.randn``) for the initial state, then one Philox seed from torch's CPU
            generator (``torch.randint``) for everything the engine draws.
"""
import torch

from .. import engine
from .._lib import DsxError


class Draws:
    def __init__(self, source, field, seed, sample_ids, B):
        """``source`` / ``field``: the sampler's ``noise_source`` / ``noise_field`` (``field`` None where the call does
        not consult it: the single steps, the objective, ``interpolate``); ``B``: the batch the ids are counted
        against.  ``streams`` is None or the checked ``(seed, ids)``."""
        self.refuse_field_with(source, field, sample_ids)             # the field's refusals come first
        self.source, self.field, self.streams = source, field, None
        if sample_ids is None:
            if seed is not None:
                raise DsxError("seed= names the per-sample noise streams: only together with sample_ids=")
            return
        if source is not None:
            raise DsxError("noise_source together with sample_ids: the draws are injected or come from the sample "
                           "streams, not both")
        if seed is None:
            raise DsxError("sample_ids need seed=: a sample stream is named by (seed, sample id)")
        self.streams = int(seed), [int(v) for v in engine._sample_ids(sample_ids, B)]

    @staticmethod
    def refuse_field_with(source, field, sample_ids):
        """``noise_field`` provides every draw of a call or none: refused together with the two other sources."""
        if field is None:
            return
        if source is not None:
            raise DsxError("noise_field together with noise_source: the draws come from one or the other")
        if sample_ids is not None:
            raise DsxError("noise_field together with sample_ids: the draws come from the field or from the sample "
                           "streams, not both")

    def normal(self, shape, device):
        """One draw of the injected or default source: the next ``noise_source`` call, else the device generator."""
        if self.source is not None:
            return self.source(tuple(shape)).to(device=device, dtype=torch.float32)
        return torch.randn(tuple(shape), device=device)

    def _asked(self, shape, draw, device):
        """Draw ``draw`` of ``noise_field`` for a state of ``shape``."""
        shape = tuple(int(v) for v in shape)
        z = self.field(shape, int(draw))
        if not torch.is_tensor(z) or not z.is_cuda or z.dtype != torch.float32 or tuple(z.shape) != shape:
            raise DsxError(f"noise_field(shape, draw) must return a float32 CUDA tensor of shape {shape}")
        return z.to(device)

    def _philox_seed(self):
        """The Philox seed of what the engine draws itself: from torch's CPU generator by default; 0, and no draw from
        that generator, where the noise is injected."""
        if self.source is not None or self.field is not None:
            return 0
        return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())

    def initial(self, shape, device):
        """The initial state, draw 0."""
        if self.field is not None:
            return self._asked(shape, 0, device)
        if self.streams is not None:
            return engine.randn_samples(shape, *self.streams, draw=0, device=device)
        return self.normal(shape, device)

    def loop(self, shape, n_rows, rows, device):
        """The keywords ``noise=``, ``seed=`` (and ``sample_ids=``) of an engine loop of ``n_rows`` rows of which
        ``rows`` add noise.  Field and injected draws travel as ``noise`` (n_rows, B, C, H, W): step ``s`` holds draw
        ``s + 1``, a row that does not draw stays zero and keeps its ordinal.  ``noise`` is None where the device
        draws or no row does; a default run in which no row draws takes seed 0 and leaves torch's generator alone."""
        rows = list(rows)
        if self.streams is not None:
            return dict(noise=None, seed=self.streams[0], sample_ids=self.streams[1])
        noise = None
        if rows and (self.field is not None or self.source is not None):
            noise = torch.zeros((n_rows,) + tuple(shape), device=device)
            for s in rows:
                noise[s] = self._asked(shape, s + 1, device) if self.field is not None else self.normal(shape, device)
        return dict(noise=noise, seed=self._philox_seed() if rows else 0)

    def per_sample(self, shape, n_rows, device):
        """``(initial state, loop keywords)`` of a loop with one start time per sample, every row drawing.  The
        reference runs such samples one at a time, so a ``noise_source`` is asked sample by sample -- the start draw,
        then one draw per step, each of shape (1, C, H, W); every other source draws as ``initial`` and ``loop`` do."""
        if self.source is None:
            return self.initial(shape, device), self.loop(shape, n_rows, range(n_rows), device)
        one = (1,) + tuple(shape[1:])
        starts, steps = [], []
        for _ in range(shape[0]):
            starts.append(self.normal(one, device))
            steps.append(torch.cat([self.normal(one, device) for _ in range(n_rows)]))
        return torch.cat(starts), dict(noise=torch.stack(steps, dim=1).contiguous(), seed=0)   # (n_rows, B, C, H, W)

    def step(self, shape, device, draw=None, noise=None):
        """The noise keywords of a single step (``engine.posterior_step`` / ``q_sample``): ``seed=``, ``sample_ids=``
        and the ordinal ``draw=`` under streams; else ``z=`` -- the caller's ``noise`` or one injected draw of
        ``shape`` -- with seed 0, or ``z=None`` and a fresh Philox seed."""
        if self.streams is not None:
            return dict(seed=self.streams[0], sample_ids=self.streams[1], draw=draw)
        if noise is None and self.source is not None:
            noise = self.normal(shape, device)
        if noise is not None:
            return dict(z=noise.to(device=device, dtype=torch.float32).contiguous(), seed=0)
        return dict(z=None, seed=self._philox_seed())
