"""Per-frame content / style strength of the UnZipLoRA delta.

Every row of a spatial projection belongs to one (batch element, frame).  A `LoraGate` holds two fp32 gates per such
row, g_content and g_style, and the projection scales the content and style columns of its LoRA down-projection
u = bf16(x Acat^T) by them: u' = bf16(g * float(u)) (kernels.linear_lora(gate=...), kernels.lora_gate).  Columns that
belong to neither key (zero padding, plain LoRA and temporal LoRA factors) take gate 1.

The object owns static device buffers: the [rows, 2] table and, per distinct column layout (`ProjOps.keys`; a handful
per model), the expanded [rows, P] table the kernels read.  `set` rewrites all of them in place, so a captured step
that holds their addresses sees the new values on its next replay; `version` counts the rewrites (the attention
processor re-projects the text K/V it cached under an older version).
"""
from __future__ import annotations

import weakref
from typing import Sequence

import torch

CONTENT, STYLE, UNGATED = 0, 1, -1


def gate_values(value, rows: int, name: str) -> torch.Tensor:
    """A scalar or a [rows] sequence -> finite fp32 CPU tensor [rows]; ValueError otherwise."""
    t = torch.as_tensor(value, dtype=torch.float32).detach().cpu()
    if t.dim() == 0:
        t = t.expand(rows)
    if t.dim() != 1 or t.shape[0] != rows:
        raise ValueError(f"{name} gate: shape {tuple(t.shape)}, expected a scalar or ({rows},)")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} gate: values must be finite")
    return t.contiguous()


class LoraGate:
    def __init__(self, rows: int, device=None):
        if rows <= 0:
            raise ValueError(f"LoraGate: {rows} rows")
        self.rows = int(rows)
        self.table = torch.ones(self.rows, 2, dtype=torch.float32, device=device)
        self.version = 0
        self._expanded = {}   # keys tuple -> (column index [P], fp32 [rows, P])
        self._text = []       # [(weakref(enc), enc version, repeated text rows)]

    @property
    def device(self):
        return self.table.device

    def set(self, content=1.0, style=1.0):
        """New gate values for every row (scalars or [rows]), validated before anything is written."""
        c = gate_values(content, self.rows, "content")
        s = gate_values(style, self.rows, "style")
        self.table.copy_(torch.stack([c, s], 1))
        for idx, t in self._expanded.values():
            self._fill(idx, t)
        self.version += 1
        return self

    def _fill(self, idx, t):
        src = torch.cat([self.table, torch.ones(self.rows, 1, dtype=torch.float32, device=self.device)], 1)
        t.copy_(src[:, idx])

    def expanded(self, keys: Sequence[int]) -> torch.Tensor:
        """fp32 [rows, len(keys)]: column c holds table[:, keys[c]], 1 where keys[c] is UNGATED.  One buffer per
        layout, kept for the life of the object."""
        keys = tuple(int(k) for k in keys)
        hit = self._expanded.get(keys)
        if hit is None:
            if len(keys) % 4 or any(k not in (CONTENT, STYLE, UNGATED) for k in keys):
                raise ValueError(f"LoraGate: column keys {keys}")
            idx = torch.tensor([2 if k < 0 else k for k in keys], dtype=torch.long, device=self.device)
            t = torch.empty(self.rows, len(keys), dtype=torch.float32, device=self.device)
            self._fill(idx, t)
            hit = self._expanded[keys] = (idx, t)
        return hit[1]

    def text_rows(self, enc: torch.Tensor) -> torch.Tensor:
        """[rows * L, D]: the text states of every gate row (enc [be, L, D] repeated over the rows // be frames of
        each batch element), made once per text and shared by every attn2 layer."""
        be, L, D = enc.shape
        if self.rows % be:
            raise ValueError(f"LoraGate: {self.rows} rows over {be} text batches")
        for ref, ver, rep in self._text:
            if ref() is enc and ver == enc._version:
                return rep
        rep = enc.repeat_interleave(self.rows // be, 0).reshape(self.rows * L, D).contiguous()
        self._text[:] = [c for c in self._text if c[0]() is not None] + [(weakref.ref(enc), enc._version, rep)]
        return rep
