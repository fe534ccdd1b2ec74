"""Training the CRNN mask estimators (disco_theque/dnn/engine/train.py, dnn/utils.py:143-186 and :249-294, dnn/engine/callbacks.py) with
the data, the loss and the recurrent layer on the GPU: batches come out of a SpectraBank (dnn/data.py), the network runs through
CRNN.forward_train and the loss through recon_loss_frames (dnn/losses.py).  The convolutions, BatchNorm, the GEMMs and RMSprop are
PyTorch-ROCm's, with its autograd.

    python -m disco_amd.dnn.train --time-step      one training step, this route against CRNN.forward (nn.GRU) + the loss as a torch expression
"""
import argparse
import json
import os
import string
import time

import numpy as np
import torch
from torch import nn

from . import data as _data
from .crnn import CRNN
from .losses import recon_loss_frames, reconstruction_loss
from .utils import get_x_for_loss


def load_architecture(n_ch, win_len=21, **kwargs):
    """(model, optimizer) as the reference builds them (dnn/utils.py:143-152, models/crnn.py:105-106): the CRNN of tango.py's load_models
    in train mode, RMSprop(lr=0.001) with `.clip = False`."""
    model = CRNN(n_ch=n_ch, win_len=win_len)
    optimizer = torch.optim.RMSprop(model.parameters(), lr=0.001)
    optimizer.clip = False
    return model, optimizer


def load_states(model, optimizer, saved_states, device=None):
    """Load a checkpoint (a path, or the dictionary itself) with the keys 'model_state_dict', 'optimizer_state_dict', 'train_loss' and
    'val_loss' into `model` and `optimizer` (dnn/utils.py:155-175); the model goes to `device` (default: a GPU if there is one) before the
    optimizer state is loaded.  Returns the loss histories with their trailing zeros trimmed."""
    device = ('cuda' if torch.cuda.is_available() else 'cpu') if device is None else device
    states = saved_states if isinstance(saved_states, dict) else torch.load(saved_states, map_location=device, weights_only=False)
    model.load_state_dict(states['model_state_dict'])
    model.to(device)
    optimizer.load_state_dict(states['optimizer_state_dict'])
    return np.trim_zeros(np.asarray(states['train_loss']), 'b'), np.trim_zeros(np.asarray(states['val_loss']), 'b')


def get_model_name(model_name):
    """A four-character name off the clock, or `<previous>_retrain` (dnn/utils.py:178-186)."""
    if model_name is None:
        chars = string.ascii_letters + string.digits
        return ''.join(chars[int(str(time.time())[-4:]) % len(chars)] for _ in range(4))
    return model_name.split('/')[-1].split('_model')[0] + '_retrain'


class SaveAndStop:
    """Says whether a value is the best so far (save the model) and whether it has not improved for more than `patience` queries (stop):
    dnn/engine/callbacks.py, whose early_stop_query does not parse as shipped; this is its evident meaning."""

    def __init__(self, patience=np.inf, mode='min', delta=0):
        if mode not in ('min', 'max'):
            raise ValueError('`mode` can be only "min" or "max"')
        self.waited, self.patience, self.mode, self.delta = 0, patience, mode, delta
        self.current_value = np.inf if mode == 'min' else -np.inf

    def save_model_query(self, value):
        better = value < self.current_value - self.delta if self.mode == 'min' else value > self.current_value + self.delta
        if better:
            self.current_value, self.waited = value, 0
        else:
            self.waited += 1
        return bool(better)

    def early_stop_query(self):
        return self.waited > self.patience


def _loss_of(model, x, y, output_frames):
    ff_in = model.get_loss_frames(output_frames)[0][0]
    return recon_loss_frames(model.forward_train(x, output_frames), y, x, ff_in)


def train_one_batch(model, x, y, optimizer, output_frames='last'):
    """One training step (dnn/utils.py:249-273): x (B, n_ch, W, F) or (B, W, F) un-normed input, y (B, W, F) label -> the loss value.
    Train mode, forward_train + recon_loss_frames, backward, clip_grad_norm_(1) where optimizer.clip is set, optimizer.step()."""
    model.train()
    loss_value = _loss_of(model, x, y, output_frames)
    optimizer.zero_grad()
    loss_value.backward()
    if getattr(optimizer, 'clip', False):
        nn.utils.clip_grad_norm_(model.parameters(), 1, norm_type=2)
    optimizer.step()
    return loss_value.item()


def eval_one_batch(model, x, y, output_frames='last'):
    """One evaluation step (dnn/utils.py:276-294): eval mode (running BatchNorm statistics), no gradient -> the loss value."""
    model.eval()
    with torch.no_grad():
        return _loss_of(model, x, y, output_frames).item()


def fit(model, optimizer, train_bank, val_bank, n_epochs, batch_size=500, output_frames='all', save_path='models/', state_dicts=None, rng=None,
        name=None, verbose=True):
    """The epoch loop of train.py:108-158.  state_dicts: None to start afresh, or the path of a `_model.pt` checkpoint to resume from (its
    loss histories are continued, the files get the name `<previous>_retrain`).  Per epoch: the mean training loss over data.batches(train_bank),
    the mean validation loss over val_bank, `{name}_losses.pt` ({'train_loss', 'val_loss'}, saved even without improvement) and, when the
    validation loss is the best so far, `{name}_model.pt` in the reference's format ('model_state_dict', 'optimizer_state_dict', 'train_loss',
    'val_loss') -- what build_crnn(state_dict=...) and the reference's load_states take.
    rng: numpy.random.Generator of the shuffles and draws (default: seed 26, the seed train.py sets).  Returns (train_losses, val_losses, name)."""
    rng = np.random.default_rng(26) if rng is None else rng
    device = train_bank.data.device
    if state_dicts is None:
        train_losses, val_losses = np.zeros(n_epochs), np.zeros(n_epochs)
        first_epoch = 0
        model.to(device)
    else:
        train_losses, val_losses = load_states(model, optimizer, state_dicts, device=device)
        first_epoch = len(train_losses)
        train_losses = np.concatenate((train_losses, np.zeros(n_epochs)))
        val_losses = np.concatenate((val_losses, np.zeros(n_epochs)))
    callback = SaveAndStop(patience=n_epochs, mode='min')
    os.makedirs(save_path, exist_ok=True)
    name = get_model_name(state_dicts) if name is None else name
    for i_epoch in range(first_epoch, first_epoch + n_epochs):
        train_loss = sum(train_one_batch(model, x, y, optimizer, output_frames) for x, y in _data.batches(train_bank, batch_size, rng))
        val_loss = sum(eval_one_batch(model, x, y, output_frames) for x, y in _data.batches(val_bank, batch_size, rng))
        train_losses[i_epoch] = train_loss / _data.n_batches(train_bank, batch_size)
        val_losses[i_epoch] = val_loss / _data.n_batches(val_bank, batch_size)
        if verbose:
            print('epoch {}\n\tTrain \t {} \t \t Val \t {}'.format(i_epoch, train_losses[i_epoch], val_losses[i_epoch]))
        torch.save({'train_loss': train_losses, 'val_loss': val_losses}, os.path.join(save_path, '{}_losses.pt'.format(name)))
        if callback.save_model_query(val_losses[i_epoch]):
            torch.save({'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(), 'train_loss': train_losses,
                        'val_loss': val_losses}, os.path.join(save_path, name + '_model.pt'))
        if callback.early_stop_query():
            break
    return train_losses, val_losses, name


# ---- python -m disco_amd.dnn.train --time-step ------------------------------------------------------------------------------------------------

def _plain_step(model, x, y, optimizer, output_frames):
    """The reference's train_one_batch as the package could already run it: CRNN.forward (nn.GRU) and the loss as a torch expression."""
    model.train()
    est = model(x)
    loss_value = reconstruction_loss(get_x_for_loss(y, output_frames, model=model, model_output=0),
                                     get_x_for_loss(est, output_frames, model=model, model_output=1),
                                     get_x_for_loss(x, output_frames, model=model, model_output=0))
    optimizer.zero_grad()
    loss_value.backward()
    optimizer.step()
    return loss_value.item()


def time_step(n_ch_list=(1, 4), batch_size=500, output_frames='all', steps=30, warmup=5, rounds=3, device='cuda:0'):
    """Wall time of one training step on seeded random banks, two ways on the same batches: 'plain' (_plain_step) and 'new'
    (train_one_batch).  Both end in loss.item(), a device synchronise, so a host clock around `steps` steps measures finished work; every
    shape is warmed up first, and the two routes alternate over `rounds` rounds so that drift of the machine shows as spread, not as a
    difference.  The batch gather is timed on its own.  Needs a GPU: there is nothing to measure without one."""
    if not torch.cuda.is_available():
        raise RuntimeError('--time-step measures the GPU: no GPU is visible')
    out = []
    for n_ch in n_ch_list:
        g = torch.Generator(device='cpu').manual_seed(11)
        K, n_seg, T, F = 4, 8, 600, 257
        S = 2 * K if n_ch == 1 else 3 * K
        spectra = torch.rand((S, n_seg, F, T), generator=g) * 2
        bank = _data.SpectraBank(spectra, stack_axis=0 if n_ch == 1 else 2, device=device)
        assert bank.n_ch == n_ch
        rng = np.random.default_rng(5)
        times = {'plain': [], 'new': [], 'gather': []}
        routes = {}
        for route in ('plain', 'new'):
            torch.manual_seed(3)
            model, opt = load_architecture(n_ch)
            routes[route] = (model.to(device), opt)
        tabs = [bank.draw_batch(rng.integers(len(bank), size=batch_size), rng) for _ in range(4)]
        batches_ = [bank.gather(t) for t in tabs]
        batches_ = [((x[:, 0].contiguous() if n_ch == 1 else x), y) for x, y in batches_]

        def run(route, n):
            model, opt = routes[route]
            step = _plain_step if route == 'plain' else train_one_batch
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(n):
                x, y = batches_[i % len(batches_)]
                step(model, x, y, opt, output_frames)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / n

        for route in ('plain', 'new'):
            run(route, warmup)
        for _ in range(rounds):
            for route in ('plain', 'new'):
                times[route].append(run(route, steps))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                bank.gather(tabs[i % len(tabs)])
            torch.cuda.synchronize()
            times['gather'].append((time.perf_counter() - t0) / steps)
        med = {k: float(np.median(v)) for k, v in times.items()}
        out.append({'n_ch': n_ch, 'batch_size': batch_size, 'output_frames': output_frames, 'steps': steps, 'rounds': rounds,
                    'plain_ms': 1e3 * med['plain'], 'new_ms': 1e3 * med['new'], 'plain_over_new': med['plain'] / med['new'],
                    'gather_ms': 1e3 * med['gather'], 'plain_ms_all': [1e3 * t for t in times['plain']],
                    'new_ms_all': [1e3 * t for t in times['new']]})
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description='Training of the CRNN mask estimators')
    p.add_argument('--time-step', action='store_true', help='time one training step (B = 500, all frames, n_ch 1 and 4): nn.GRU route against the new one')
    p.add_argument('--steps', type=int, default=30)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--batch-size', type=int, default=500)
    args = p.parse_args(argv)
    if not args.time_step:
        p.error('nothing to do: --time-step (training itself is driven from Python: load_architecture, SpectraBank.from_rooms or .from_files, fit)')
    for rec in time_step(steps=args.steps, rounds=args.rounds, batch_size=args.batch_size):
        print(json.dumps(rec))


if __name__ == '__main__':
    main()
