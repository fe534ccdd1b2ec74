"""Training data of the mask estimators, held on the device (disco_theque/dnn/data/datasets.py, DiscoDataset): the magnitudes of every
segment's signals in one bank, the reference's choice of window / local node / compressed signals per item as small index tables drawn on
the host, and the windows gathered into a batch by one kernel (disco_train_batch).  A training loop copies nothing to the device but
those tables.  The bank is filled from the reference's .npy training set (SpectraBank.from_files) or straight from rooms on the device
(SpectraBank.from_rooms: step 1 of the path and one fill kernel, disco_bank_fill; no files).

The reference draws from the global np.random stream inside DataLoader worker processes, which is not reproducible; here every draw comes
from a numpy.random.Generator the caller passes in, and that stream is not imitated."""
import numpy as np
import torch

FS = 16000                              # datasets.py:7
Z_OUTPUTS = {'zs_hat': 'z_y', 'zn_hat': 'zn'}       # a z signal's name in the training set -> the step-1 output it is (speech_enhancement/z_dataset.py)


def _check_stack_axis(stack_axis):
    if stack_axis == 1:
        raise NotImplementedError('stack_axis=1 (channels stacked along frequency) is not offered: 0 or 2, the values train.py uses')
    if stack_axis not in (0, 2):
        raise ValueError('`stack_axis` should be 0 (SC) or 2 (MC stacked over the channels)')


def _z_outputs(z_sigs):
    """None, 'zs_hat', 'zn_hat' or a list of the two -> the step-1 outputs they are, in that order."""
    names = [] if z_sigs is None else ([z_sigs] if isinstance(z_sigs, str) else list(z_sigs))
    if any(nm not in Z_OUTPUTS for nm in names) or len(set(names)) != len(names):
        raise ValueError(f"z_sigs: None, 'zs_hat', 'zn_hat' or a list of the two expected, got {z_sigs!r}")
    return [Z_OUTPUTS[nm] for nm in names]


def _rooms_of(a, r0, count):
    """Rooms [r0, r0 + count) of an (R, ...) array as a contiguous view: a DevBuf by its `part`, NumPy arrays and tensors by a slice."""
    if int(a.shape[0]) == count:
        return a
    if hasattr(a, 'part'):
        shape = (count,) + tuple(int(v) for v in a.shape[1:])
        return a.part(r0 * int(np.prod(shape[1:], dtype=np.int64)), shape)
    return a[r0:r0 + count]


class SpectraBank:
    """(S, N, T, F) float32 magnitudes on a device: S signal rows x N segments, frequency innermost as everywhere else in the package, and
    n_frames (N,), the frames each segment has (the rest of a row is zeros, as load_data leaves it).
    Row order is that of the reference's `segs_to_load` (get_input_lists): K reference-microphone mixtures, then K rows per z signal, then
    the K masks last.
    data: arrays or tensors in the reference's (S, N, F, T) orientation, complex or real, host or device: abs is taken and the last two axes
    are swapped.  n_frames: None = all T.  stack_axis: 0 (single-channel network: the local mixture only) or 2 (multi-channel: the z signals
    of the other nodes stacked as channels), the two values train.py uses; 1 (stacked along frequency) is not offered.
    z_nodes: None = min(stack_axis, 1) (K - 1), as the reference."""

    def __init__(self, data, n_frames=None, n_nodes=4, stack_axis=0, z_nodes=None, win_len=21, win_hop=8, device=None):
        _check_stack_axis(stack_axis)
        t = data if torch.is_tensor(data) else torch.from_numpy(np.ascontiguousarray(data))
        if device is not None:
            t = t.to(device)
        if t.dim() != 4:
            raise ValueError(f'data: (S, N, F, T) expected, got {tuple(t.shape)}')
        self._adopt(t.abs().to(torch.float32).transpose(2, 3).contiguous(), n_frames, n_nodes, stack_axis, z_nodes, win_len, win_hop)

    @classmethod
    def _from_bank_layout(cls, data, n_frames, n_nodes=4, stack_axis=0, z_nodes=None, win_len=21, win_hop=8):
        """A bank around a ready (S, N, T, F) float32 tensor (from_rooms: filled on the device by disco_bank_fill): taken as it is, no abs /
        transpose pass over it."""
        _check_stack_axis(stack_axis)
        if data.dim() != 4 or data.dtype != torch.float32 or not data.is_contiguous():
            raise ValueError(f'bank layout: a contiguous float32 (S, N, T, F) tensor expected, got {data.dtype} {tuple(data.shape)}')
        self = object.__new__(cls)
        self._adopt(data, n_frames, n_nodes, stack_axis, z_nodes, win_len, win_hop)
        return self

    def _adopt(self, data, n_frames, n_nodes, stack_axis, z_nodes, win_len, win_hop):
        self.data = data
        self.S, self.N, self.T, self.F = self.data.shape
        self.n_nodes, self.stack_axis, self.win_len, self.win_hop = int(n_nodes), stack_axis, int(win_len), int(win_hop)
        if self.S % self.n_nodes or self.S < 2 * self.n_nodes:
            raise ValueError(f'{self.S} signal rows: K mixtures, K rows per z signal and K masks expected (K = {self.n_nodes})')
        self.n_zsig = self.S // self.n_nodes - 2
        self.z_nodes = min(stack_axis, 1) * (self.n_nodes - 1) if z_nodes is None else int(z_nodes)
        if not 0 <= self.z_nodes <= self.n_nodes - 1:
            raise ValueError(f'z_nodes in [0, {self.n_nodes - 1}] expected')
        self.n_ch = 1 + self.z_nodes * self.n_zsig
        self.n_frames = np.full(self.N, self.T, np.int64) if n_frames is None else np.asarray(n_frames, np.int64).reshape(-1)
        if self.n_frames.shape[0] != self.N or self.n_frames.min() < self.win_len or self.n_frames.max() > self.T:
            raise ValueError(f'n_frames: {self.N} values in [{self.win_len}, {self.T}] expected')
        self.win_per_seg = (self.n_frames - self.win_len) // self.win_hop + 1
        self.n_cum = np.concatenate(([0], np.cumsum(self.win_per_seg)))

    @classmethod
    def from_files(cls, lists_to_load, skip_frames=None, fs=FS, hop=256, device=None, **kwargs):
        """From lists of .npy files as get_input_lists and speech_enhancement/z_dataset.py produce them: lists_to_load[i_sig][i_seg], every
        file an (F, T_seg) spectrogram.  The first skip_frames frames are dropped -- default ceil(fs / hop), the reference's silent first
        second (datasets.py:72, 81) --, a segment's frame count is that of its row 0, shorter rows are zero-filled (load_data)."""
        skip = int(np.ceil(fs / hop)) if skip_frames is None else int(skip_frames)
        S, N = len(lists_to_load), len(lists_to_load[0])
        rows = [[np.abs(np.load(lists_to_load[i][j]))[:, skip:] for j in range(N)] for i in range(S)]
        F, T = rows[0][0].shape[0], max(r.shape[1] for sig in rows for r in sig)
        data = np.zeros((S, N, F, T), np.float32)
        for i in range(S):
            for j in range(N):
                data[i, j, :, :rows[i][j].shape[1]] = rows[i][j]
        return cls(data, n_frames=[rows[0][j].shape[1] for j in range(N)], device=device, **kwargs)

    @classmethod
    def from_rooms(cls, y, s, n, lengths=None, z_sigs='zs_hat', ref_channel=1, mask_type='irm1', skip_frames=None, fs=FS, n_fft=512,
                   rooms_per_call=None, **bank_kwargs):
        """From rooms, without leaving the device and without files: y, s, n (R, K, M, L) float32 -- NumPy arrays, or DevBufs / device tensors as
        dataset_utils.mix_rooms and meeting_rooms return them -- become the bank of R segments that from_files builds from the reference's
        training set of the same rooms (dataset_utils.post.write_post_dataset + speech_enhancement.z_dataset.write_z_dataset).
        Step 1 runs through Engine.tango_reference(steps=1) on a cached engine with its own oracle masks of `mask_type` at microphone
        ref_channel - 1 (1 ... M, as get_input_lists counts): its masks_z are the label rows, its z_y ('zs_hat') / zn ('zn_hat') the z rows;
        z_sigs: None, one of the two names, or a list of them (rows in the list's order).  The mixture rows are the spectra of that microphone
        from one Engine.stft of y in the node groups the path itself transforms (channel pairs share a transform, so a channel's bits depend
        on its group: these are the spectra the masks were computed beside).  disco_bank_fill writes magnitudes and masks into the bank.
        lengths: (R,) valid samples per room (Engine.set_lengths), T_r = 1 + lengths[r] // hop.  The first skip_frames frames are dropped
        (None: ceil(fs / hop), the reference's silent first second); n_frames[r] = T_r - skip_frames, the bank's T is their maximum.
        rooms_per_call: rooms per engine call (None: all R at once); the pieces fill one bank.  bank_kwargs: stack_axis, z_nodes, win_len,
        win_hop, n_nodes (default K).  ValueError, before anything is launched: a room with fewer than win_len frames left, a mask_type outside
        the irm / ibm / iam families, ref_channel outside 1 ... M."""
        from .._engines import get_engine
        from ..engine import parse_mask_type
        unknown = set(bank_kwargs) - {'stack_axis', 'z_nodes', 'win_len', 'win_hop', 'n_nodes'}
        if unknown:
            raise TypeError(f'from_rooms: unexpected keyword(s) {sorted(unknown)}')
        parse_mask_type(mask_type)
        _check_stack_axis(bank_kwargs.get('stack_axis', 0))
        if len(y.shape) != 4 or tuple(s.shape) != tuple(y.shape) or tuple(n.shape) != tuple(y.shape):
            raise ValueError(f'y, s, n: three (R, K, M, L) arrays expected, got {tuple(y.shape)}, {tuple(s.shape)}, {tuple(n.shape)}')
        R, K, M, L = (int(v) for v in y.shape)
        if not 1 <= int(ref_channel) <= M:
            raise ValueError(f'ref_channel {ref_channel}: 1 ... {M} expected (the microphones of a node)')
        outputs = _z_outputs(z_sigs)
        hop = n_fft // 2
        skip = int(np.ceil(fs / hop)) if skip_frames is None else int(skip_frames)
        if skip < 0:
            raise ValueError(f'skip_frames {skip}: not negative expected')
        lens = np.full(R, L, np.int64) if lengths is None else np.asarray(lengths).reshape(-1).astype(np.int64)
        if lens.shape[0] != R or (lengths is not None and not np.array_equal(lens, np.asarray(lengths).reshape(-1))) or lens.min() < 1 or lens.max() > L:
            raise ValueError(f'lengths: {R} integers in [1, {L}] expected')
        frames = 1 + lens // hop
        n_frames = frames - skip
        win_len = int(bank_kwargs.get('win_len', 21))
        short = np.flatnonzero(n_frames < win_len)
        if short.size:
            r = int(short[0])
            raise ValueError(f'room {r}: {int(frames[r])} frames - {skip} skipped leave {int(n_frames[r])}, fewer than one window of {win_len}')
        per_call = R if rooms_per_call is None else int(rooms_per_call)
        if per_call < 1:
            raise ValueError(f'rooms_per_call {rooms_per_call}: at least 1 expected')
        S, Tb, bank = K * (2 + len(outputs)), int(n_frames.max()), None
        for r0 in range(0, R, per_call):
            Rp = min(per_call, R - r0)
            eng = get_engine(rooms=Rp, nodes=K, mics=M, length=L, n_fft=n_fft, mask=mask_type, pad_mode='reflect', ref_mic=int(ref_channel) - 1,
                             mu=1.0, staged_step2=True)
            if bank is None:            # where the engine's pointers live: its GPU (a test's emulated library: host memory)
                bank = torch.empty((S, R, Tb, eng.F), dtype=torch.float32, device='cpu' if eng._host_pointers_ok else f'cuda:{eng.cfg.device}')
            try:                        # (a cached engine: the lengths do not outlive the call)
                if lengths is not None:
                    eng.set_lengths(lens[r0:r0 + Rp])
                yd, sd, nd = (eng.to_device(_rooms_of(a, r0, Rp), np.float32)[1] for a in (y, s, n))
                out = eng.tango_reference(yd, sd, nd, steps=1, want=outputs + ['masks_z'])
                X = eng.stft(yd.reshape(Rp * K, M, L))
                fr = None if lengths is None else eng.to_device(frames[r0:r0 + Rp].astype(np.int32), np.int32)[1]
                z = [out[nm].ptr for nm in outputs] + [None, None]
                eng._chk(eng.lib.disco_bank_fill(eng.ctx, X.ptr, z[0], z[1], out['masks_z'].ptr, None if fr is None else fr.ptr, Rp, K, M, eng.T,
                                                 eng.F, int(ref_channel) - 1, len(outputs), skip, bank.data_ptr(), R, Tb, r0, eng.stream))
                eng.sync()              # the sources are freed when this iteration ends
            finally:
                if lengths is not None:
                    eng.set_lengths(None)
        bank_kwargs.setdefault('n_nodes', K)
        return cls._from_bank_layout(bank, n_frames, **bank_kwargs)

    def windows_per_segment(self):
        """(N,) windows of win_len frames at hop win_hop each segment holds (datasets.py:85)."""
        return self.win_per_seg

    def __len__(self):
        return int(self.win_per_seg.sum())

    def item_indices(self, item, jitter):
        """(segment k, first frame m) of `item` (get_item_indices, datasets.py:105-118) for a jitter in [0, win_hop): k from the cumulative
        window counts, m = min((item - n_cum[k]) win_hop + jitter, n_frames[k] - win_len).  item, jitter: ints or arrays."""
        item = np.asarray(item, np.int64)
        if item.size and (item.min() < 0 or item.max() >= len(self)):
            raise IndexError(f'item in [0, {len(self)}) expected')
        k = np.searchsorted(self.n_cum, item, side='right') - 1
        m = np.minimum((item - self.n_cum[k]) * self.win_hop + np.asarray(jitter, np.int64), self.n_frames[k] - self.win_len)
        return k, m

    def draw_batch(self, items, rng):
        """The index table of a batch, int32 (B, C + 3): per item (k, m, the C input rows, the label row) (__getitem__ / get_subwindow,
        datasets.py:92-162).  Per item, from `rng`: the jitter, the local node uniform over K, and for z_nodes == 1 which other node's
        compressed signal it receives.  Input rows: the local mixture, then K (i_sig + 1) + z_chs[i_ch] ordered by i_ch, then i_sig, with
        z_chs = roll(arange(K), K - 1 - local)[:z_nodes], i.e. (local + 1 + i_ch) mod K.  Label row: S - K + local."""
        items = np.asarray(items, np.int64).reshape(-1)
        B, K = items.shape[0], self.n_nodes
        k, m = self.item_indices(items, rng.integers(self.win_hop, size=B))
        local = rng.integers(K, size=B)
        tab = np.empty((B, self.n_ch + 3), np.int32)
        tab[:, 0], tab[:, 1], tab[:, 2], tab[:, -1] = k, m, local, self.S - K + local
        first = 1 + rng.integers(K - 1, size=B) if self.z_nodes == 1 else np.ones(B, np.int64)        # a random one of the other nodes
        for i_ch in range(self.z_nodes):
            z_ch = (local + first + i_ch) % K
            for i_sig in range(self.n_zsig):
                tab[:, 3 + i_ch * self.n_zsig + i_sig] = K * (i_sig + 1) + z_ch
        return tab

    def check_table(self, tab):
        tab = np.ascontiguousarray(tab, np.int32)
        if tab.ndim != 2 or tab.shape[1] != self.n_ch + 3 or tab.shape[0] < 1:
            raise ValueError(f'table: (B, {self.n_ch + 3}) expected, got {tab.shape}')
        return tab

    def gather(self, tab):
        """The windows of an index table: x (B, C, W, F) and y (B, W, F) float32 on the bank's device, through disco_train_batch (a bank on
        the CPU: by index, in torch).  A table with a segment, a window (m + W > T) or a signal row out of range raises ValueError before
        anything is launched."""
        from .crnn import _DeviceOf, _stream_of, _use_kernels
        tab = self.check_table(tab)
        B, C, W = tab.shape[0], self.n_ch, self.win_len
        if not _use_kernels(self.data):
            if (tab[:, 0].min() < 0 or tab[:, 0].max() >= self.N or tab[:, 1].min() < 0 or tab[:, 1].max() > self.T - W or tab[:, 2:].min() < 0
                    or tab[:, 2:].max() >= self.S):
                raise ValueError('table entry out of range (segment, m + W > T, or signal row)')
            t = torch.from_numpy(tab.astype(np.int64))
            xy = self.data[t[:, 2:, None], t[:, 0, None, None], (t[:, 1, None] + torch.arange(W))[:, None, :]]
            return xy[:, :C].contiguous(), xy[:, C].contiguous()
        from .. import _lib
        dev = self.data.device
        x = torch.empty((B, C, W, self.F), dtype=torch.float32, device=dev)
        y = torch.empty((B, W, self.F), dtype=torch.float32, device=dev)
        tab_dev = torch.from_numpy(tab).to(dev)
        with _DeviceOf(self.data):
            rc = _lib.load().disco_train_batch(None, self.data.data_ptr(), self.S, self.N, self.T, self.F, tab_dev.data_ptr(), tab.ctypes.data, B, C, W,
                                               x.data_ptr(), y.data_ptr(), _stream_of(self.data))
        if rc == _lib.E_ARG:
            raise ValueError('table entry out of range (segment, m + W > T, or signal row)')
        if rc != 0:
            raise RuntimeError(f'disco_train_batch failed ({rc})')
        return x, y


def batches(bank, batch_size, rng, shuffle=True):
    """One epoch over `bank` as the reference's DataLoader(DiscoDataset) delivers it: (x, y) device tensors, x (B, C, W, F) -- (B, W, F)
    for C == 1 --, y (B, W, F); every item once, in a permutation from `rng` if shuffle; the last batch may be short."""
    order = rng.permutation(len(bank)) if shuffle else np.arange(len(bank))
    for i in range(0, len(order), batch_size):
        x, y = bank.gather(bank.draw_batch(order[i:i + batch_size], rng))
        yield (x[:, 0] if bank.n_ch == 1 else x), y


def n_batches(bank, batch_size):
    return -(-len(bank) // batch_size)
