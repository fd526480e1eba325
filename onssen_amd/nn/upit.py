import torch
import torch.nn as nn

from .. import options
from ._train import head_linear
from ._core import (PackedWeightsMixin, needs_graph, BLSTMParams, PackedBLSTM, PackedHead, _Workspaces, EPI_SIGMOID, as_frames,
                    heads_take_image, require_device, run_blstm, run_head, use_hip_path)


class uPIT_LSTM(PackedWeightsMixin, nn.Module):
    """Drop-in for the reference's uPIT_LSTM (onssen/nn/uPIT-LSTM.py: a file upstream cannot import, its name has a hyphen): same
    constructor, parameter names and shapes (rnn.*, fc_mi.{weight, bias}; ``embedding_dim`` is unused, as upstream).

    forward([x (B,T,F)]) -> ``num_speaker`` masks (B,T,output_dim), strided views of one contiguous (B,T,output_dim,S) buffer laid
    out as upstream's reshape lays it.  Upstream returns the first two slices whatever ``num_speaker`` is; returning all S is
    the extension, and for S = 2 the result is upstream's.  ``masks(x)`` returns the buffer itself."""

    def __init__(self, input_dim, output_dim, hidden_dim=300, embedding_dim=20, num_layers=3, dropout=0.5, num_speaker=2,
                 **hip_options):
        super().__init__()
        options.constructor_options(type(self).__name__, hip_options)      # optional config keys (precision, recurrence, ...)
        self.input_dim, self.output_dim, self.hidden_dim = input_dim, output_dim, hidden_dim
        self.embedding_dim, self.num_layers, self.num_speaker = embedding_dim, num_layers, num_speaker
        self.add_module("rnn", BLSTMParams(input_dim, hidden_dim, num_layers, dropout))
        self.add_module("fc_mi", nn.Linear(hidden_dim * 2, output_dim * num_speaker))
        self._packed = PackedBLSTM(self.rnn)
        self._head = PackedHead(self.fc_mi, None, hidden_dim)
        self._ws = _Workspaces()
        self._init_packed_hooks()

    def forward(self, input, frames=None):
        """``frames`` (extension; inference only): per-row frame counts of a ragged batch of whole utterances, as in
        ``chimera.forward`` -- row b's masks inside its own frames are bit for bit its batch-1 result."""
        assert len(input) == 1, "There must be one tensor in the input for the uPIT network"
        x = input[0].float()
        if not use_hip_path(self) or needs_graph(*input):
            if frames is not None:
                raise RuntimeError("uPIT_LSTM: frames=... (ragged batch) is an inference-path extension")
            m = self._autograd_forward(x)
        else:
            m = self.masks(x, frames)
        return [m[..., k] for k in range(self.num_speaker)]

    def masks(self, x, frames=None):
        """HIP inference path: x (B,T,F) -> masks (B,T,output_dim,S), ``forward``'s list as one buffer."""
        x = x.float()
        batch_size, frame, _ = x.size()
        require_device(x, "uPIT_LSTM")
        if frames is not None:
            frames = as_frames(frames, batch_size, frame, x.device)
        y = run_blstm(self._packed, self._ws, x, frames=frames, need_y=not heads_take_image(batch_size, self.hidden_dim))
        m = run_head(self._head, y, batch_size, frame, EPI_SIGMOID)                    # (B, T, output_dim * S)
        return m.view(batch_size, frame, self.output_dim, self.num_speaker)

    def _autograd_forward(self, x):
        B, T, _ = x.shape
        r = self.rnn.autograd_forward(x, self.training)
        return torch.sigmoid(head_linear(self.fc_mi, r)).reshape(B, T, self.output_dim, self.num_speaker)
