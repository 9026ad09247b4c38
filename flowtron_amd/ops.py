"""torch.autograd.Function wrappers around the C ABI (include/flowtron_hip.h).

Each Function's forward AND backward enqueue hand-written HIP kernels on torch's
current stream through ctypes; torch supplies device memory and the autograd
graph only.  Nothing here computes on the CPU and nothing falls back to torch
ops for the math: a missing library or a CPU tensor raises.

Layouts (reference flowtron.py internal layout after :884): activations are
time-major [T,B,C] fp32 contiguous; lengths are int32 device tensors.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence

import torch

from . import _lib as L

# --------------------------------------------------------------------------
# raw launchers
# --------------------------------------------------------------------------


def _c(t: torch.Tensor) -> torch.Tensor:
    return t if t.is_contiguous() else t.contiguous()


import os as _os
_BF16_IMAGES = True        # large 16-bit GEMMs run from shared operand images (round 1; the switch was retired in round 6)


def gemm_raw(A, B, Cm, M, N, K, sAm, sAk, sBk, sBn, ldc, bias=None, act=L.ACT_NONE, alpha=1.0, beta=0.0,
             batch=1, bsA=0, bsB=0, bsC=0, mode=None, splitk=False):
    """C = act(alpha*A.B + beta*C + bias); A,B,Cm are tensors whose data_ptr is the operand origin.
    splitk=True (weight-gradient GEMMs only) allows the atomic split-K path."""
    L.require_cuda(A, B, Cm, bias)
    a = L.GemmArgs(L.ptr(A), L.ptr(B), L.ptr(Cm), L.ptr(bias), M, N, K, batch,
                   sAm, sAk, sBk, sBn, ldc, bsA, bsB, bsC, alpha, beta, act,
                   L.mfma_mode() if mode is None else mode, L.GEMM_SPLITK if splitk else 0,
                   None, 0)
    if _BF16_IMAGES:
        need = L.lib().ft_gemm_workspace_bytes(C.byref(a))
        if need:                      # large bf16-mode GEMM: bf16 operand images + DMA-staged kernel (gemm_bf16.hip)
            work = torch.empty(need, device=Cm.device, dtype=torch.uint8)     # stream-ordered by the caching allocator
            a.work, a.work_bytes = L.ptr(work), need
    L.check(L.lib().ft_gemm(C.byref(a), L.stream()), "ft_gemm")


# --------------------------------------------------------------------------
# bf16 operand images (csrc/gemm_bf16.hip): every fp32 matrix that feeds a large bf16-mode GEMM is rounded ONCE and the
# image serves all its GEMMs -- x: forward + dW, dY: dX + dW, W: forward + dX, LSTM dgates: dW_hh + dW_ih (+ dX) --
# k-contiguous or k-major as the GEMM needs (k-major fragments come from the LDS transpose-read, so nothing is transposed).
# --------------------------------------------------------------------------
class RowMap:
    """Pack-by-length row map of the time-major decoder activations [T,B,*] (csrc: ft_rowmap_build; the reference packs with
    pack_padded_sequence, flowtron.py:689-694): compact rows are batch-major, utterance b = its valid frames + ONE separator
    (its first padded frame, or a zero row when it has none).  Built on the device from the int32 length vector -- no host
    sync; `cap` = T*B + B is the capacity images and grids are sized for, `rows` the device-side row count."""
    __slots__ = ("T", "B", "cap", "lens", "map", "rows", "gather")

    def __init__(self, lens32, T, B):
        L.require_cuda(lens32)
        self.T, self.B, self.cap, self.lens = int(T), int(B), int(T) * int(B) + int(B), lens32
        self.map = torch.empty(self.cap, device=lens32.device, dtype=torch.int32)
        self.rows = torch.empty(1, device=lens32.device, dtype=torch.int32)
        L.check(L.lib().ft_rowmap_build(L.ptr(lens32), L.ptr(self.map), L.ptr(self.rows), self.T, self.B, L.stream()), "ft_rowmap_build")

    def fill(self, y2d, ncols, copy_separator):
        """padded frames t > len_b of the time-major matrix y2d [T*B, >= ncols]: zeros, or (copy_separator) the values of the
        utterance's first padded frame, which a compact GEMM has just computed"""
        L.check(L.lib().ft_pad_rows_fill(L.ptr(y2d), int(y2d.stride(0)), int(ncols), L.ptr(self.lens), self.T, self.B,
                                         1 if copy_separator else 0, L.stream()), "ft_pad_rows_fill")


_COMPACT = _os.environ.get("FLOWTRON_GEMM_COMPACT", "1") != "0"
_FUSE_ACT_BWD = True       # activation backward inside the gradient's image pass (round 4)
# split-K on the encoder's FORWARD split-image GEMM (160 output tiles, K = 7 680).  With fp32 atomics (the first form: the
# first form, -0.2 ms per step) the order of the atomics makes the forward itself differ from run to run (z up to 8e-4, bf16 gradients
# up to 1e-2 rel-L2 on the same batch and weights: scripts/exp/noise_debug.py, profiles/r05b_forward_noise.log).  Default "det": the
# slices' partial products side by side + a fixed-order reduction (FT_GEMM_SPLITK_DET) -- a forward pass is a function of its inputs;
# "0": one slice
_ENC_SPLITK = "det"
_CAT_IMAGES = True         # a Linear over two inputs as ONE GEMM over a concatenated image (round 4)
_PERSIST_IMG = _os.environ.get("FLOWTRON_LSTM_PERSIST_IMG", "1")      # 1: the persistent backward emits the dgates image INSTEAD of fp32 dgx where its only consumer is the projection's backward; both; 0


def row_map(lens32, T, B):
    """the RowMap the 16-bit image GEMMs of a [T,B,*] stack should use, or None (FLOWTRON_GEMM_COMPACT=0: padded rows are multiplied)"""
    return RowMap(lens32, T, B) if (_COMPACT and _BF16_IMAGES) else None


class Bf16Image:
    __slots__ = ("buf", "rows", "cols", "ld", "colsum", "fmt", "rowmap")

    def __init__(self, t2d, colsum=False, mode=None, rowmap=None):
        """t2d: fp32 CUDA matrix [rows, cols], unit column stride.  colsum=True also returns the fp32 column sums of t2d
        (self.colsum) from the same pass -- the bias gradient when t2d is an output gradient.
        rowmap: a RowMap over t2d's rows (t2d = a time-major [T*B, cols] activation): the image holds the VALID rows only, in
        compact order (self.rows = the map's capacity)."""
        assert t2d.dim() == 2 and t2d.stride(1) == 1 and t2d.dtype == torch.float32
        L.require_cuda(t2d)
        self.rows, self.cols = int(t2d.shape[0]), int(t2d.shape[1])
        self.fmt = L.mfma_mode() if mode is None else mode      # FT_BF16 or FT_F16: 16-bit payloads of that operand format
        self.ld = (self.cols + 255) // 256 * 256
        self.rowmap = rowmap
        # column sums (bias gradients) are ADDED to a zeroed slice of the backward pass's slab (the _acc entry points: no memset each)
        self.colsum = zeroed((self.cols,), t2d.device) if colsum else None
        if rowmap is not None:
            assert self.rows == rowmap.T * rowmap.B, "row map built for another [T, B]"
            self.rows = rowmap.cap
            self.buf = torch.empty(L.lib().ft_bf16_image_bytes(self.rows, self.cols), device=t2d.device, dtype=torch.uint8)
            L.check(L.op16("ft_bf16_image_rows_acc", self.fmt)(L.ptr(t2d), int(t2d.stride(0)), self.rows, self.cols, L.ptr(self.buf), L.ptr(self.colsum),
                                                                L.ptr(rowmap.map), L.ptr(rowmap.rows), L.stream()), "ft_bf16_image_rows_acc")
            return
        self.buf = torch.empty(L.lib().ft_bf16_image_bytes(self.rows, self.cols), device=t2d.device, dtype=torch.uint8)
        if colsum:
            L.check(L.op16("ft_bf16_image_colsum_acc", self.fmt)(L.ptr(t2d), int(t2d.stride(0)), self.rows, self.cols, L.ptr(self.buf), L.ptr(self.colsum),
                                                     L.stream()), "ft_bf16_image_colsum_acc")
        else:
            L.check(L.op16("ft_bf16_image", self.fmt)(L.ptr(t2d), int(t2d.stride(0)), self.rows, self.cols, L.ptr(self.buf), L.stream()), "ft_bf16_image")

    def ptr(self, row_off=0, col_off=0):
        assert col_off % 8 == 0
        return self.buf.data_ptr() + 2 * (row_off * self.ld + col_off)

    def view_cols(self, cols):
        """the first `cols` columns as an image of their own (same storage and row stride): the [hi] block of a split image IS the
        plain image of the matrix"""
        v = Bf16Image.__new__(Bf16Image)
        v.buf, v.rows, v.cols, v.ld, v.colsum, v.fmt, v.rowmap = self.buf, self.rows, int(cols), self.ld, None, self.fmt, self.rowmap
        return v

    @classmethod
    def split3(cls, t2d, mode, weight):
        """[hi | lo | hi] (activation) / [hi | hi | lo] (weight) image of t2d [rows, K]: one 16-bit GEMM over 3 K columns then gives
        x w to ~u16^2 (ft_bf16_image_split3; measured 4e-6 of sum |x w| in bf16 and 4e-7 in fp16 at the encoder's weight scale against
        1.4e-3 and 2e-4 from [hi] alone -- fp16's lo of a weight is subnormal, and below |w| ~ 1e-3 that floor is all that is left:
        csrc/gemm_bf16.hip, tests/conv_ref64.py)"""
        assert t2d.dim() == 2 and t2d.stride(1) == 1 and t2d.dtype == torch.float32 and t2d.shape[1] % 8 == 0
        self = cls.__new__(cls)
        self.rows, self.cols, self.fmt, self.rowmap, self.colsum = int(t2d.shape[0]), 3 * int(t2d.shape[1]), mode, None, None
        self.ld = (self.cols + 255) // 256 * 256
        self.buf = torch.empty(L.lib().ft_bf16_image_bytes(self.rows, self.cols), device=t2d.device, dtype=torch.uint8)
        L.check(L.op16("ft_bf16_image_split3", mode)(L.ptr(t2d), int(t2d.stride(0)), self.rows, int(t2d.shape[1]), L.ptr(self.buf),
                                                     1 if weight else 0, L.stream()), "ft_bf16_image_split3")
        return self

    @classmethod
    def split3_im2col(cls, x, lens, KW, mode):
        """the [hi | lo | hi] image of ft_im2col(x, lens, KW) -- x [L, B, C] -- made straight from x (ft_bf16_image_split3_im2col): the
        fp32 column matrix is never written"""
        Lx, B, Cc = x.shape
        self = cls.__new__(cls)
        self.rows, self.cols, self.fmt, self.rowmap, self.colsum = int(Lx * B), 3 * int(Cc * KW), mode, None, None
        self.ld = (self.cols + 255) // 256 * 256
        self.buf = torch.empty(L.lib().ft_bf16_image_bytes(self.rows, self.cols), device=x.device, dtype=torch.uint8)
        L.check(L.op16("ft_bf16_image_split3_im2col", mode)(L.ptr(x), L.ptr(lens), int(Lx), int(B), int(Cc), int(KW), L.ptr(self.buf), L.stream()),
                "ft_bf16_image_split3_im2col")
        return self

    @classmethod
    def _blank(cls, rows, cols, mode, device):
        self = cls.__new__(cls)
        self.rows, self.cols, self.fmt, self.rowmap, self.colsum = int(rows), int(cols), mode, None, None
        self.ld = (self.cols + 255) // 256 * 256
        self.buf = torch.empty(L.lib().ft_bf16_image_bytes(self.rows, self.cols), device=device, dtype=torch.uint8)
        return self

    @classmethod
    def of_weight(cls, W, mode, split=False):
        """the (plain | split [hi | hi | lo]) image of a WEIGHT matrix.  Inside a Flowtron.forward (weight_images_begin) the images of
        all weights the previous forward of that model asked for are rounded in ONE launch at the first request
        (ft_bf16_image_table: 23 dispatches of 5-15 us -> 1) -- from the CURRENT values, every forward anew: nothing is cached across
        steps (a weight changed through `.data` would not bump its version).  Outside, or for a weight not in the plan: one launch."""
        w = _WIMG
        key = (W.data_ptr(), tuple(W.shape), mode, bool(split))
        if w["plan_next"] is not None:
            w["plan_next"][key] = W
        if w["armed"]:
            w["armed"] = False
            # (a planned tensor whose storage moved since the previous forward -- FlatArena flattening after the first forward, a p.data
            #  swap -- or changed shape is dropped: its image would sit under a stale key that no request finds, or that a same-shape
            #  tensor reusing the old address could pick up)
            plan = [(k, t) for k, t in w["plan"].items() if t.is_cuda and t.device == W.device and t.dtype == torch.float32 and t.is_contiguous()
                    and t.data_ptr() == k[0] and tuple(t.shape) == k[1]]
            for lo in range(0, len(plan), 32):
                part = plan[lo:lo + 32]
                by_fmt = {}
                for k, t in part:
                    by_fmt.setdefault(k[2], []).append((k, t))
                for fmt, items in by_fmt.items():
                    descs = (L.ImgDesc * len(items))()
                    for i, (k, t) in enumerate(items):
                        img = cls._blank(t.shape[0], (3 if k[3] else 1) * t.shape[1], fmt, t.device)
                        descs[i] = L.ImgDesc(t.data_ptr(), int(t.stride(0)), int(t.shape[0]), int(t.shape[1]), img.buf.data_ptr(), 1 if k[3] else 0)
                        w["cache"][k] = img
                    L.check(L.op16("ft_bf16_image_table", fmt)(descs, len(items), L.stream()), "ft_bf16_image_table")
        img = w["cache"].get(key)
        if img is not None:
            return img
        return cls.split3(W, mode, True) if split else cls(W, mode=mode)

    @classmethod
    def cat_rows(cls, xs2d, mode, rowmap):
        """ONE compact image of the column-wise concatenation [x_0 | x_1 | ..] of time-major activations (each [T*B, K_i] fp32,
        K_i % 8 == 0 except the last): a Linear over several inputs then runs as one GEMM with one K loop (flowtron.py:758-765
        concatenates [h_att ; ctx] before the decoder LSTM), and its weight gradient as one split-K GEMM."""
        self = cls.__new__(cls)
        self.rows, self.cols, self.fmt, self.rowmap, self.colsum = rowmap.cap, int(sum(x.shape[1] for x in xs2d)), mode, rowmap, None
        self.ld = (self.cols + 255) // 256 * 256
        self.buf = torch.empty(L.lib().ft_bf16_image_bytes(self.rows, self.cols), device=xs2d[0].device, dtype=torch.uint8)
        off = 0
        for i, x in enumerate(xs2d):
            assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float32 and x.shape[0] == rowmap.T * rowmap.B
            K = int(x.shape[1])
            last = i == len(xs2d) - 1
            assert last or K % 8 == 0
            L.check(L.op16("ft_bf16_image_rows_into", mode)(L.ptr(x), int(x.stride(0)), self.rows, K, L.ptr(self.buf), self.ld, off,
                                                            (self.ld - off) if last else K, L.ptr(rowmap.map), L.ptr(rowmap.rows), L.stream()),
                    "ft_bf16_image_rows_into")
            off += K
        return self

    @classmethod
    def empty_rows(cls, cols, rowmap, mode, device):
        """an UNWRITTEN compact image over `rowmap` ([cap, cols] 16-bit payloads of format `mode`) with zeroed column sums, for a
        kernel that produces the image itself (ft_lstm_persist_bwd_img)"""
        self = cls.__new__(cls)
        self.rows, self.cols, self.fmt, self.rowmap = rowmap.cap, int(cols), mode, rowmap
        self.ld = (self.cols + 255) // 256 * 256
        self.buf = torch.empty(L.lib().ft_bf16_image_bytes(self.rows, self.cols), device=device, dtype=torch.uint8)
        self.colsum = zeroed((self.cols,), device)
        return self


# weight images of one forward pass in one launch (Bf16Image.of_weight): the plan = what the previous forward of the same model asked for
_WIMG_ON = True
_WIMG = {"plan": {}, "plan_next": None, "cache": {}, "armed": False, "plans": None,
         # the same for the recurrences' W_hh fragment images (roles_wimg): key -> [weight, its backward image is wanted too]
         "wf_plan": {}, "wf_plan_next": None, "wf_cache": {}, "wf_armed": False, "wf_plans": None, "wf_last": None, "wf_grad": False}


def weight_images_begin(model):
    """called at the head of Flowtron.forward: arm the one-launch conversion of the weights this model's previous forward used"""
    if not _WIMG_ON:
        return
    w = _WIMG
    if w["plans"] is None:
        w["plans"], w["wf_plans"] = _weakref.WeakKeyDictionary(), _weakref.WeakKeyDictionary()
    w["plan"] = w["plans"].get(model, {})
    w["plan_next"], w["cache"], w["armed"] = {}, {}, bool(w["plan"])
    w["wf_plan"] = w["wf_plans"].get(model, {})
    w["wf_plan_next"], w["wf_cache"], w["wf_armed"], w["wf_last"] = {}, {}, bool(w["wf_plan"]), None
    w["wf_grad"] = torch.is_grad_enabled()       # (read HERE: the requests come from inside autograd Functions, where it is off)


def weight_images_end(model):
    w = _WIMG
    if w["plan_next"] is not None and w["plans"] is not None:
        w["plans"][model] = w["plan_next"]
    w["plan"], w["plan_next"], w["cache"], w["armed"] = {}, None, {}, False
    if w["wf_plan_next"] is not None and w["wf_plans"] is not None:
        w["wf_plans"][model] = w["wf_last"] = w["wf_plan_next"]      # (the pass's backward marks the entries whose backward image it asks for)
    # forward images not taken are dropped here; backward images wait for this pass's backward
    w["wf_cache"] = {k: v for k, v in w["wf_cache"].items() if k[1]}
    w["wf_plan"], w["wf_plan_next"], w["wf_armed"] = {}, None, False


# images of activations are shared between every consumer of the SAME tensor (h_att feeds the query projection, the gate and
# the decoder input projection; an LSTM output also feeds its own dW_hh GEMM in backward): keyed by tensor identity
# (id + weakref + version), dropped with the tensor.
import weakref as _weakref
_IMG_CACHE = {}


def shared_image(t, rows, cols, mode, rowmap=None):
    """16-bit image (operand format `mode`) of the fp32 tensor `t` viewed as [rows, cols]; one conversion per tensor (version)
    and row map."""
    key = id(t)
    hit = _IMG_CACHE.get(key)
    want_rows = rows if rowmap is None else rowmap.cap
    if hit is not None:
        ref, ver, img = hit
        if ref() is t and ver == t._version and img.rows == want_rows and img.cols == cols and img.fmt == mode and img.rowmap is rowmap:
            return img
    img = Bf16Image(t.reshape(rows, cols), mode=mode, rowmap=rowmap)
    if len(_IMG_CACHE) > 64:                     # dead entries (their tensors are gone) are swept lazily
        for k in [k for k, (r, _, _) in _IMG_CACHE.items() if r() is None]:
            del _IMG_CACHE[k]
    try:
        _IMG_CACHE[key] = (_weakref.ref(t, lambda _r, k=key: _IMG_CACHE.pop(k, None)), t._version, img)
    except TypeError:
        pass
    return img


def op16_dtype(mode):
    """torch dtype of a tensor that holds 16-bit values of the operand format `mode`"""
    return torch.float16 if mode == L.FT_F16 else torch.bfloat16


_GX16 = True     # gx of the persistent forward recurrences as 16-bit rows (round 6; tests set it False to compare with fp32 rows)


def gx16_ok(mode, rowmap, T, B, H, reverse, xs, N, device):
    """whether an input projection may write its output as 16-BIT rows (FT_GEMM_C16): its only reader is a persistent forward recurrence
    (csrc/lstm_roles.hip takes them) and its gradient travels back as the dgates image alone (so the fp32 face autograd would
    otherwise round to 16 bits never carries values)"""
    return (_GX16 and L.is16(mode) and rowmap is not None and not reverse and rowmap.T == T and rowmap.B == B and _PERSIST_IMG == "1"
            and linear_uses_images(mode, T * B, N, xs) and (len(xs) == 1 or _CAT_IMAGES)
            and B <= 32 and lstm_persistent(B, H, reverse, mode, device))


def images_apply(mode, M, N, K):
    """same rule as ft_gemm_workspace_bytes: bf16 mode and a GEMM large enough to amortise the image passes."""
    return _BF16_IMAGES and L.is16(mode) and M >= 32 and N >= 32 and K >= 16 and M * N * K >= (1 << 20)


def _gemm_img_args(A, a_km, a_ptr, B, b_km, b_ptr, Cm, M, N, K, ldc, bias=None, act=L.ACT_NONE, alpha=1.0, beta=0.0, splitk=False,
                   rowmap=None, compact=0, k_shift=0, rank1=None, c16=False, a_rows=None, split_work_bytes=None):
    """the ft_gemm_img_args of gemm_img's arguments, and the split-K workspace they point into (to be kept alive by the caller)"""
    L.require_cuda(Cm, bias)
    flags, work, need = (L.GEMM_SPLITK if splitk else 0), None, 0
    if splitk == "det":
        # deterministic split-K (forward GEMMs): partial products side by side in a workspace, added in a fixed order
        need = L.lib().ft_gemm_img_split_work_bytes(M, N, K)
        if split_work_bytes is not None:         # a smaller workspace than asked for: the call runs as many slices as it holds
            need = min(need, int(split_work_bytes))
        flags = L.GEMM_SPLITK_DET if need else 0
        work = torch.empty(need, device=Cm.device, dtype=torch.uint8) if need else None
    if c16:                                      # C is a 16-bit tensor of the operands' format (FT_GEMM_C16)
        assert Cm.dtype == op16_dtype(A.fmt) and not splitk and beta == 0.0
        flags |= L.GEMM_C16
    a = L.GemmImgArgs(a_ptr, b_ptr, L.ptr(Cm), L.ptr(bias), M, N, K, A.ld, B.ld, ldc, int(a_km), int(b_km),
                      alpha, beta, act, flags,
                      L.ptr(rowmap.map) if rowmap is not None else None, L.ptr(rowmap.rows) if rowmap is not None else None,
                      int(compact) if rowmap is not None else 0, int(k_shift),
                      L.ptr(rank1[0]) if rank1 is not None else None, rank1[1] if rank1 is not None else None,
                      L.ptr(work), need, L.ptr(a_rows) if a_rows is not None else None)
    assert A.fmt == B.fmt, "operand images of different formats"
    return a, work


def gemm_img(A, a_km, a_ptr, B, b_km, b_ptr, Cm, M, N, K, ldc, **kw):
    """C[M,N] = act(alpha * A.B + beta*C + bias) from images.  a_ptr / b_ptr: A.ptr(...) / B.ptr(...) (may point inside).
    Keywords: bias, act, alpha, beta, splitk (True: atomic split-K allowed; "det": the deterministic form, split_work_bytes = a
    smaller workspace than the library asks for), c16 (Cm is a 16-bit tensor of the operands' format), and
    rowmap + compact: 1 = M runs over the map's compact rows (pass M = rowmap.cap), C rows are scattered through the map;
    2 = the reduction runs over compact rows (pass K = rowmap.cap; k_shift = a row shift already applied to a_ptr).
    rank1 = (r [C rows] fp32, c_ptr -> N floats): C[row][col] += r[row] * c[col] in the epilogue (row = the output row).
    a_rows (int32 device list, compact = 1): compact row m reads row a_rows[m] of A's image instead of row m."""
    a, _work = _gemm_img_args(A, a_km, a_ptr, B, b_km, b_ptr, Cm, M, N, K, ldc, **kw)
    L.check(L.op16("ft_gemm_img", A.fmt)(C.byref(a), L.stream()), "ft_gemm_img")


def gemm_img_plan(A, a_km, a_ptr, B, b_km, b_ptr, Cm, M, N, K, ldc, **kw):
    """what gemm_img would launch with the same arguments (ft_gemm_img_plan: the launcher's own decision, nothing is launched):
    a GemmImgPlan (tile_rows, stage_k, gather, atomics, det, splits, chunk_w)"""
    a, _work = _gemm_img_args(A, a_km, a_ptr, B, b_km, b_ptr, Cm, M, N, K, ldc, **kw)
    plan = L.GemmImgPlan()
    L.check(L.lib().ft_gemm_img_plan(C.byref(a), C.byref(plan)), "ft_gemm_img_plan")
    return plan


# Weight-gradient GEMMs of a backward pass in grouped launches (ft_gemm_img_group).  Nothing in the backward chain reads a weight
# gradient, so the image-path dW GEMMs wait in a per-pass queue and run together: one grid per tile height instead of ~31 launches
# that each fill the chip once and end on ~512 partial tiles of atomics.  A queued problem holds the buffers of both operand images, the row map
# and an alias of C until it has run; every image of a pass is a fresh allocation that no later kernel writes again (the hand-off and
# shared_image only pass references on, the pair backward's windows have all written their dgates images before its weight gradients
# are queued), so holding the reference is all the lifetime a queued operand needs -- at the price of the images staying allocated
# to the end of the pass.
# The queue runs (a) from an engine callback queued with the first deferred problem of the pass, (b) when the table is full, (c) from
# flush_weight_grads(), which whoever reads gradients before the pass ends calls first (dist: a bucket's all-reduce).
# A problem is deferred only where the tensor it writes is the one autograd will adopt as .grad without reading it: the weight is a
# leaf (or a reshape of one) without a gradient yet, without tensor hooks, met for the first time in the pass, outside anomaly mode and
# double backward.  Everything else -- and everything outside a backward pass, or with _DW_GROUP = False -- launches at once, and a
# later gradient of a weight whose first one waits runs the queue first (_dw_other_gradient).  By construction outside this module:
# a weight that ALSO feeds a foreign autograd node in the same pass would have its two gradients added before the queue has run.
_DW_GROUP = True
_DWQ = {"task": None, "items": [], "seen": {}}


def _dw_leaf(W):
    """the leaf whose .grad the gradient of W becomes through reshapes alone, or None where that cannot be told"""
    if W.is_leaf:
        return W
    b = W._base
    if b is not None and b.is_leaf and b.numel() == W.numel() and W.is_contiguous() and b.is_contiguous():
        return b
    return None


def _dw_end_of_pass():
    flush_weight_grads()
    _DWQ["task"], _DWQ["seen"] = None, {}


def _dw_pass():
    """the queue state of the current backward pass, armed at its first use (as _handoff_put does: keyed by the engine's graph task,
    the leftovers of a pass that raised are dropped, never launched); None outside a pass and wherever nothing is deferred"""
    if not _DW_GROUP or torch.is_grad_enabled() or torch.is_anomaly_enabled():
        return None
    gt = _current_graph_task()
    if gt == -1:
        return None
    q = _DWQ
    if q["task"] != gt:
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_dw_end_of_pass)
        except RuntimeError:
            return None
        q["task"], q["items"], q["seen"] = gt, [], {}
    return q


def _dw_deferrable(W, dW):
    """whether this weight-gradient GEMM may wait for the flush"""
    q = _dw_pass()
    if q is None or W is None:
        return False
    leaf = _dw_leaf(W)
    if leaf is None or not leaf.requires_grad or leaf.grad is not None or leaf._backward_hooks:
        return False
    first = q["seen"].setdefault(id(leaf), dW.data_ptr())
    if first != dW.data_ptr():
        flush_weight_grads()            # a second gradient of one weight in the pass: the engine adds the two, so the first must be there
        return False
    return True


def _dw_other_gradient(W):
    """A gradient of W is about to be produced OUTSIDE the queue (an fp32-staging GEMM, a scatter-add, zeros).  A weight may be used
    more than once in a pass -- a batch wider than the recurrence kernels runs its layers per batch chunk, and a chunk may be too
    small for the image path -- and the engine adds the gradients of one weight as soon as the later one arrives: one that still
    waits in the queue is written first, and one that comes after this one will not wait (address 0 matches no C).  Every other
    producer of a gradient for a weight that can also reach weight_grad_gemm (LinearFn and the recurrences) calls this."""
    q = _dw_pass()
    leaf = _dw_leaf(W) if (q is not None and W is not None) else None
    if leaf is None:
        return
    if id(leaf) in q["seen"]:
        flush_weight_grads()
    q["seen"][id(leaf)] = 0


def weight_grad_gemm(W, dW, A, a_ptr, B, b_ptr, Cm, M, N, K, ldc, **kw):
    """The image-path weight-gradient GEMM Cm (+)= A^T B (both images k-major, gemm_img's arguments with splitk = True), Cm = dW or a
    column window of it, dW = the gradient the node returns for the weight W.  Inside a backward pass the call joins the pass's queue
    (see above) and runs with the others in ft_gemm_img_group; else it is gemm_img itself."""
    if not _dw_deferrable(W, dW):
        gemm_img(A, 1, a_ptr, B, 1, b_ptr, Cm, M, N, K, ldc, splitk=True, **kw)
        return
    a, _work = _gemm_img_args(A, 1, a_ptr, B, 1, b_ptr, Cm, M, N, K, ldc, splitk=True, **kw)
    # (the images' buffers, not the images, and an alias of C, not C: autograd adopts a returned gradient -- C here, an image's column
    #  sums as a bias gradient -- without a copy only while nobody else holds that tensor)
    _DWQ["items"].append((a, A.fmt, L.stream(), Cm.device, (A.buf, B.buf, Cm.detach(), kw.get("rowmap"), kw.get("bias"))))
    if len(_DWQ["items"]) >= L.GEMM_GROUP_MAX:
        flush_weight_grads()


def gemm_img_group(arg_list, fmt, stream=None):
    """ft_gemm_img_group over a list of ft_gemm_img_args (at most L.GEMM_GROUP_MAX) of operand format fmt"""
    arr = (L.GemmImgArgs * len(arg_list))(*arg_list)
    L.check(L.op16("ft_gemm_img_group", fmt)(arr, len(arg_list), L.stream() if stream is None else stream), "ft_gemm_img_group")


def gemm_img_group_plan(arg_list):
    """what gemm_img_group would launch: one L.GemmImgGroupPlan per problem (ft_gemm_img_group_plan; nothing is launched)"""
    arr = (L.GemmImgArgs * len(arg_list))(*arg_list)
    out = (L.GemmImgGroupPlan * len(arg_list))()
    L.check(L.lib().ft_gemm_img_group_plan(arr, len(arg_list), out), "ft_gemm_img_group_plan")
    return list(out)


def _dw_run(batch):
    """one ft_gemm_img_group call over queue items (args, format, stream, device, kept references) of one format, stream and device"""
    with torch.cuda.device(batch[0][3]):
        gemm_img_group([it[0] for it in batch], batch[0][1], batch[0][2])


def flush_weight_grads():
    """run every weight-gradient GEMM the current backward pass has deferred; after it the gradients produced so far are complete.
    Call it before reading a gradient inside a pass (a hook, a collective over finished buckets)."""
    items, _DWQ["items"] = _DWQ["items"], []
    gt = _current_graph_task()
    if gt != -1 and gt != _DWQ["task"]:
        return                          # leftovers of a pass that raised, met inside a later pass: dropped, never launched
    while items:
        fmt, st, dev = items[0][1:4]
        batch = [it for it in items if it[1:4] == (fmt, st, dev)][:L.GEMM_GROUP_MAX]
        taken = set(id(it) for it in batch)
        items = [it for it in items if id(it) not in taken]
        _dw_run(batch)


# hand-off of an output-gradient image between two autograd nodes of the SAME backward pass (the LSTM backward builds the
# image of dgates for its own dW_hh GEMM; the input projection's LinearFn.backward receives that very tensor as dy).
# Keyed by (device, data_ptr, shape); cleared by an engine callback at the end of the pass, so an address can never match stale data.
_HANDOFF = {"imgs": {}, "armed": False, "unwritten": set(), "nan_next": 0}
_NAN_POOL = {}          # device -> 64 fp32 NaNs: one slot per image-only gradient alive in a backward pass


def _current_graph_task():
    try:
        return torch._C._current_graph_task_id()
    except Exception:                   # older torch: fall back to "one pass at a time" (the pre-round-5 behaviour)
        return -1


def _handoff_clear():
    _HANDOFF["imgs"].clear()
    _HANDOFF["unwritten"].clear()
    _HANDOFF["armed"] = False
    _HANDOFF["nan_next"] = 0


def image_only_gradient(shape, device, dtype=torch.float32):
    """The fp32 face of a gradient that exists ONLY as a 16-bit operand image (ft_lstm_persist_bwd_img): every element reads NaN.
    No storage of the gradient's size is allocated -- ONE NaN float, expanded with zero strides; each such gradient of a backward
    pass takes its own slot of a small pool, so (device, data_ptr, shape) still identifies it for the image hand-off.  A foreign
    reader (a node hook, anomaly mode's output check, an unexpected second consumer) therefore sees NaN -- never stale memory."""
    pool = _NAN_POOL.get(device)
    if pool is None:
        pool = _NAN_POOL[device] = torch.full((64,), float("nan"), device=device, dtype=torch.float32)
    i = _HANDOFF["nan_next"]
    _HANDOFF["nan_next"] = i + 1
    if dtype != torch.float32:
        # (a 16-bit face -- the gradient of 16-bit gx rows: its own pool of that dtype, the slot index keeps the address unique)
        pool = _NAN_POOL.get((device, dtype))
        if pool is None:
            pool = _NAN_POOL[(device, dtype)] = torch.full((64,), float("nan"), device=device, dtype=dtype)
    slot = pool[i:i + 1] if i < 64 else torch.full((1,), float("nan"), device=device, dtype=dtype)
    return slot.expand(*shape) if len(shape) else slot.reshape(())


def _handoff_put(t, img, key=None):
    # one clear callback per backward PASS.  The engine drops its callbacks when a backward raises, which used to leave `armed`
    # set for good: imgs / unwritten / nan_next were then never cleared again.  A pass is identified by the engine's
    # current graph task; a put from another pass than the one that armed the state clears the leftovers and arms again.
    gt = _current_graph_task()
    if not _HANDOFF["armed"] or _HANDOFF.get("task") != gt:
        if _HANDOFF["armed"]:
            _handoff_clear()
        try:
            torch.autograd.Variable._execution_engine.queue_callback(_handoff_clear)
        except RuntimeError:            # not inside a backward pass: no consumer can follow
            return
        _HANDOFF["armed"] = True
        _HANDOFF["task"] = gt
    _HANDOFF["imgs"][(t.device.index, t.data_ptr(), tuple(t.shape) if key is None else key)] = img


def _handoff_put_x(x, img):
    """the operand image a Linear's backward has just used for its INPUT x, left for the node that produced x: an LSTM's backward
    multiplies the same compact image of its output (dW_hh = dgates^T . y shifted by one row) and would otherwise convert y again"""
    if img is not None and img.rowmap is not None:
        _handoff_put(x, img, key=("x", x.numel()))


def _handoff_take_x(y, cols, mode, rowmap):
    img = _HANDOFF["imgs"].get((y.device.index, y.data_ptr(), ("x", y.numel()))) if _HANDOFF["armed"] else None
    if img is not None and img.rowmap is rowmap and img.fmt == mode and img.cols == cols and img.rows == rowmap.cap:
        return img
    return None


def y_image(y, rows, cols, mode, rowmap):
    """the compact image of an LSTM output for its own weight-gradient GEMM: the one a consumer's backward left (same pass), else made here"""
    img = _handoff_take_x(y, cols, mode, rowmap) if rowmap is not None else None
    return img if img is not None else shared_image(y, rows, cols, mode, rowmap)


def _handoff_take(t):
    return _HANDOFF["imgs"].pop((t.device.index, t.data_ptr(), tuple(t.shape)), None)


def _handoff_put_image_only(t, img):
    """as _handoff_put, for a gradient tensor whose fp32 storage was NOT written (only its image exists): a consumer that would
    read the fp32 values fails loudly (_require_written)"""
    _handoff_put(t, img)
    if not _HANDOFF["armed"]:
        raise RuntimeError("flowtron_amd: an image-only gradient outside a backward pass")
    _HANDOFF["unwritten"].add((t.device.index, t.data_ptr(), tuple(t.shape)))


def _require_written(t):
    if _HANDOFF["unwritten"] and (t.device.index, t.data_ptr(), tuple(t.shape)) in _HANDOFF["unwritten"]:
        raise RuntimeError("flowtron_amd: this gradient exists only as a 16-bit operand image (ft_lstm_persist_bwd_img); its consumer "
                           "must take the image (set FLOWTRON_LSTM_PERSIST_IMG=both to keep the fp32 copy)")


# Split-K weight-gradient GEMMs accumulate with fp32 atomics into an output that must start at zero.  One memset per output was 37
# dispatches per training step (hipMemset2DAsync / zeros_like: 0.28 ms of ~5 us fills, profiles/r04_final_step_timeline.txt);
# the outputs of a backward pass now come out of ONE zeroed allocation sized by the previous pass's demand, and the GEMMs run with
# beta = 1 ("C holds the addend").  (_ZSLAB_ON = False: one zeroed tensor per output.)
_ZSLAB = {"buf": None, "off": 0, "need": 0, "last": 0, "task": None}
_ZSLAB_ON = True


def zeroed(shape, device):
    """a zero-filled fp32 tensor for an accumulating kernel; inside a backward pass a view into the pass's zeroed slab"""
    n = 1
    for d in shape:
        n *= int(d)
    gt = _current_graph_task() if _ZSLAB_ON else -1
    if gt == -1:
        return torch.zeros(shape, device=device, dtype=torch.float32)
    z = _ZSLAB
    if z["task"] != (gt, str(device)):
        z["last"], z["need"], z["off"], z["task"] = max(z["need"], 0), 0, 0, (gt, str(device))
        z["buf"] = torch.zeros(z["last"], device=device, dtype=torch.float32) if z["last"] > 0 else None
    step = (n + 63) // 64 * 64                           # 256-byte aligned slices (vector atomics / float4 epilogues)
    z["need"] += step
    if z["buf"] is not None and z["off"] + step <= z["buf"].numel():
        v = z["buf"][z["off"]:z["off"] + n].view(shape)
        z["off"] += step
        return v
    return torch.zeros(shape, device=device, dtype=torch.float32)


_ARENA_GRADS = True


def weight_grad_out(W):
    """the zero-filled fp32 output of W's weight-gradient kernel (split-K / atomic accumulation): inside a backward pass the slice of
    the flat gradient arena the parameter's .grad will live in anyway (dist.FlatArena.grad_view_for_pass: no copy into the arena
    afterwards), else a piece of the pass's zeroed slab.  (_ARENA_GRADS = False: always the slab.)"""
    if _ARENA_GRADS and _ZSLAB_ON:
        gt = _current_graph_task()
        if gt != -1:
            from .dist import arena_slot
            slot = arena_slot(W)
            if slot is not None:
                v = slot[0].grad_view_for_pass(slot[1], gt, W.shape)
                if v is not None:
                    return v
    return zeroed(W.shape, W.device)


# An activation with several consumers (h_att feeds the query projection AND the decoder LSTM's input projection; the encoder output
# feeds the key and value projections of every flow) gets one input gradient per consumer, which autograd then adds: a [T,B,1024]
# fp32 add of 340 MB of traffic per flow (49 us) for h_att.  The image-path Linear backward instead ACCUMULATES into the buffer the
# first consumer of the same tensor produced in this pass (its dX GEMM runs with beta = 1) and returns None for that input -- the
# engine hands the producer the one buffer.  Safe because the engine runs an activation's producer only after ALL its consumers,
# and because forward activations never share an address while alive.  Buffers are held weakly (a weak reference survives while
# the engine's input buffer owns the tensor and dies with it): nothing outlives its consumer, and a buffer the engine has folded
# into another tensor (a third, foreign contribution arriving first and adding ours in place) is simply not found again.
# Caveat, by construction outside this model: if a FOREIGN owner (a user hook that stores gradient tensors) keeps the first buffer
# alive AND a third contribution of another kind makes the engine replace it by an out-of-place sum, a later accumulation would
# go into the orphan -- h_att and the encoder output have image-path consumers only; _DX_INPLACE = False restores autograd's adds.
_DX_INPLACE = True
_DXACC = {"task": None, "bufs": {}}


def _dx_buffer(x):
    """(buffer for the input gradient of x, accumulate: the buffer already holds another consumer's contribution)"""
    gt = _current_graph_task() if _DX_INPLACE else -1
    if gt == -1:
        return torch.empty_like(x), False
    d = _DXACC
    if d["task"] != gt:
        d["task"], d["bufs"] = gt, {}
    key = (x.device.index, x.data_ptr(), tuple(x.shape))
    ref = d["bufs"].get(key)
    buf = ref() if ref is not None else None
    if buf is not None:
        return buf, True
    buf = torch.empty_like(x)
    d["bufs"][key] = _weakref.ref(buf)
    return buf, False


def colsum(x2d: torch.Tensor, rows: int, N: int, ld: int) -> torch.Tensor:
    out = torch.empty(N, device=x2d.device, dtype=torch.float32)
    L.check(L.lib().ft_colsum(L.ptr(x2d), L.ptr(out), rows, N, ld, L.stream()), "ft_colsum")
    return out


_LENS_CACHE = {}


def _lens_entry(lens: torch.Tensor):
    """int32 copy and element sum of a length vector, made ONCE per tensor (keyed by storage address + version): the same in_lens /
    out_lens reach the model, every flow, the three losses and their backward passes -- a copy + a reduction + a cast of four-byte
    kernels each time (~20 dispatches of ~5 us per training step)"""
    key = (lens.data_ptr(), lens._version, lens.numel(), lens.dtype, lens.device)
    e = _LENS_CACHE.get(key)
    if e is None or e[0]() is not lens:
        import weakref
        if len(_LENS_CACHE) > 64:
            _LENS_CACHE.clear()
        i32 = lens if (lens.dtype == torch.int32 and lens.is_contiguous()) else lens.to(dtype=torch.int32).contiguous()
        e = _LENS_CACHE[key] = (weakref.ref(lens), i32, {})
    return e


def lens32(lens: torch.Tensor) -> torch.Tensor:
    return _lens_entry(lens)[1]


def lens_total(lens: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """float32 device scalar sum(lens) * scale (the normalisers of the losses, flowtron.py:206-243)"""
    e = _lens_entry(lens)
    t = e[2].get(scale)
    if t is None:
        t = e[2][scale] = e[1].sum().to(torch.float32) * scale if scale != 1.0 else e[1].sum().to(torch.float32)
    return t


# --------------------------------------------------------------------------
# Linear over one or two row-blocks of the weight:  y = act(sum_i x_i W[:, off_i:off_i+K_i]^T + b)
# (nn.Linear / 1x1 Conv1d / LSTM input projection call sites, flowtron.py:568-571, :758, :767-768)
# --------------------------------------------------------------------------
def _dy_image(dy, w_img, rowmap, want_db):
    """A Linear's output gradient as (image, dy): the image its producer (an LSTM backward) handed over, where it fits this node (format
    of `w_img`, same rowmap, column sums where wanted), looked up on dy AS IT ARRIVES -- an image-only gradient is a zero-stride NaN
    tensor (image_only_gradient) that must not be materialised.  Else (None, dy as written fp32 values).  w_img None: no image taken."""
    img = _handoff_take(dy) if w_img is not None else None
    if img is not None and img.fmt == w_img.fmt and img.rowmap is rowmap and not (want_db and img.colsum is None):
        return img, dy
    _require_written(dy)
    return None, _c(dy.float())


def linear_uses_images(mode, rows, N, xs):
    """whether LinearFn runs (and differentiates) this projection through shared 16-bit operand images"""
    return all(images_apply(mode, rows, N, x.shape[-1]) for x in xs) and all((x.shape[-1] % 8 == 0) for x in xs[:-1])


class LinearFn(torch.autograd.Function):
    """rowmap (RowMap | None): the inputs are time-major [T,B,K] activations of a padded batch; in the 16-bit image path the
    GEMMs then run over the VALID rows only (the reference packs them, flowtron.py:689-694): compact images, output rows
    scattered back, weight gradients reduced over compact rows.  Rows of padded frames are NOT written unless `fill` asks:
      "y"  in fill: forward output rows of padded frames = the utterance's first padded frame (which the GEMM computes: every
                    padded frame of an utterance has the same inputs), for consumers that walk all T frames;
      "dx" in fill: input-gradient rows of padded frames = 0, for consumers that reduce over all T frames.
    Call sites whose consumers only ever touch valid frames (the recurrences, the next compact GEMM) pass fill = ""."""

    @staticmethod
    def forward(ctx, W, bias, act, mode, rowmap, fill, *xs):
        xs = [_c(x) for x in xs]
        L.require_cuda(W, *xs)
        W = _c(W)
        N, Ktot = W.shape
        rows = xs[0].numel() // xs[0].shape[-1]
        c16 = "c16" in fill                       # y as 16-bit rows for a persistent recurrence (gx16_ok: implies the image path below)
        y = torch.empty(xs[0].shape[:-1] + (N,), device=W.device, dtype=op16_dtype(mode) if c16 else torch.float32)
        # mode = one operand format, or (forward, input gradient, weight gradient): mixed formats (the encoder convolutions keep
        # fp32 operands where 16-bit rounding is amplified, model.Encoder) take the per-GEMM path without shared images
        mode_dx = mode_dw = mode
        if isinstance(mode, tuple):
            mode, mode_dx, mode_dw = mode
        split_fwd = mode == "split3"                 # forward products from [hi | lo | hi] x [hi | hi | lo] images of the backward's format
        if split_fwd:
            assert len(xs) == 1 and act == L.ACT_NONE and L.is16(mode_dx) and mode_dx == mode_dw
            x2d = xs[0].reshape(rows, Ktot)
            split_imgs = lazy = None
            if Ktot % 32 == 0 and images_apply(mode_dx, rows, N, Ktot):
                lazy = _LAZY_COLS.pop(xs[0].data_ptr(), None)     # (an Im2colFn output whose values were never written: image from ITS source)
                xi = Bf16Image.split3_im2col(*lazy, mode_dx) if lazy is not None else Bf16Image.split3(x2d, mode_dx, False)
                wi = Bf16Image.of_weight(W, mode_dx, split=True)
                # K = 3 Ktot over only (rows / 128) x (N / 128) output tiles (160 for the encoder: a sixth of the chip's workgroup slots,
                # 240 k-steps each: 130 us): split-K fills the chip -- in its deterministic form (see _ENC_SPLITK)
                gemm_img(xi, 0, xi.ptr(), wi, 0, wi.ptr(), y, rows, N, 3 * Ktot, N, bias=bias, splitk=_ENC_SPLITK)
                split_imgs = (wi.view_cols(Ktot), [xi.view_cols(Ktot)])      # their [hi] blocks serve the backward's GEMMs as they are
            else:
                _materialize_col(xs[0])
                gemm_raw(x2d, W, y, rows, N, Ktot, Ktot, 1, 1, Ktot, N, bias=bias, mode=L.FT_F32)
            mode = L.FT_F32                          # (what the rest of this node records as its forward format)
        mixed = not (mode == mode_dx == mode_dw)
        ctx.mode_dx, ctx.mode_dw = mode_dx, mode_dw
        use_img = (not mixed) and linear_uses_images(mode, rows, N, xs)
        # fp32 forward, 16-bit backward: the backward makes the operand images itself (the forward had none to share)
        ctx.lazy_img_mode = mode_dx if (mixed and mode_dx == mode_dw and linear_uses_images(mode_dx, rows, N, xs)) else None
        if rowmap is not None and (not use_img or rows != rowmap.T * rowmap.B):
            rowmap = None
        ctx.imgs = split_imgs if split_fwd else None
        ctx.cat = False
        # how the images were made, to make them again for a second backward through the graph (retain_graph: the first one releases them)
        ctx.img_kind = ("split3" if split_imgs is not None else None) if split_fwd else ("images" if use_img else None)
        ctx.lazy_src = lazy if split_fwd else None
        if use_img:
            w_img = Bf16Image.of_weight(W, mode)
            if len(xs) > 1 and rowmap is not None and _CAT_IMAGES:
                # [x_0 | x_1] as ONE compact image: one K loop over K_0 + K_1 (the 256 x 256 x 64 kernel applies at K >= 1536), one
                # weight-gradient GEMM -- instead of two K pieces accumulating through C (measured 259 + 316 us for the decoder
                # LSTM's input projection against ~330 for the single loop)
                x_cat = Bf16Image.cat_rows([x.reshape(rows, x.shape[-1]) for x in xs], mode, rowmap)
                ctx.imgs, ctx.cat = (w_img, [x_cat]), True
                gemm_img(x_cat, 0, x_cat.ptr(), w_img, 0, w_img.ptr(), y, rowmap.cap, N, Ktot, N, bias=bias, act=act, rowmap=rowmap, compact=1, c16=c16)
            else:
                x_imgs = [shared_image(x, rows, x.shape[-1], mode, rowmap) for x in xs]
                ctx.imgs = (w_img, x_imgs)          # reused by backward (dX reads W k-major, dW reads x k-major)
        off = 0
        for i, x in enumerate(xs):
            if ctx.cat or split_fwd:
                off = Ktot
                break
            K = x.shape[-1]
            last = i == len(xs) - 1
            if use_img:
                assert not c16 or len(xs) == 1
                gemm_img(x_imgs[i], 0, x_imgs[i].ptr(), w_img, 0, w_img.ptr(0, off), y, rows if rowmap is None else rowmap.cap, N, K, N,
                         bias=bias if last else None, act=act if last else L.ACT_NONE, beta=0.0 if i == 0 else 1.0,
                         rowmap=rowmap, compact=1, c16=c16)
            else:
                assert not c16, "16-bit output rows come from the image GEMMs only"
                gemm_raw(x, W[:, off:], y, rows, N, K, K, 1, 1, Ktot, N,
                         bias=bias if last else None, act=act if last else L.ACT_NONE,
                         beta=0.0 if i == 0 else 1.0, mode=mode)
            off += K
        assert off == Ktot
        if rowmap is not None and "y" in fill:
            rowmap.fill(y.reshape(rows, N), N, copy_separator=True)
        ctx.save_for_backward(W, y if act != L.ACT_NONE else None, *xs)
        ctx.act, ctx.mode, ctx.has_bias, ctx.rowmap, ctx.fill = act, mode, bias is not None, rowmap, fill
        return y

    @staticmethod
    def backward(ctx, dy):
        W, y, *xs = ctx.saved_tensors
        N, Ktot = W.shape
        rows = dy.numel() // N
        rowmap = ctx.rowmap
        if ctx.imgs is None and ctx.img_kind is not None:
            ctx.imgs = _linear_images_again(ctx, W, xs, rows)
        elif ctx.imgs is None and ctx.lazy_img_mode is not None:
            lm = ctx.lazy_img_mode
            ctx.imgs = (Bf16Image(W, mode=lm), [shared_image(x, rows, x.shape[-1], lm, rowmap) for x in xs])
        want_db = ctx.has_bias and ctx.needs_input_grad[1]
        d_img_in, dy = _dy_image(dy, ctx.imgs[0] if (ctx.act == L.ACT_NONE and ctx.imgs is not None) else None, rowmap, want_db)
        # an activated layer over a row map on the image path: dpre = dy act'(pre) is formed INSIDE the conversion pass (image + bias
        # column sums, ft_bf16_image_rows_act_bwd) -- no fp32 dpre tensor
        fuse_act = ctx.act != L.ACT_NONE and ctx.imgs is not None and rowmap is not None and _FUSE_ACT_BWD
        if ctx.act != L.ACT_NONE and not fuse_act:
            dpre = torch.empty_like(dy)
            L.check(L.lib().ft_act_bwd(L.ptr(y), L.ptr(dy), L.ptr(dpre), dy.numel(), ctx.act, L.stream()), "ft_act_bwd")
        else:
            dpre = dy
        dW = None
        if ctx.needs_input_grad[0]:
            if ctx.imgs is None:
                _dw_other_gradient(W)
            dW = weight_grad_out(W) if ctx.imgs is not None else torch.empty_like(W)      # (image path: split-K with beta = 1)
        db = None
        dxs = []
        off = 0
        imgs = ctx.imgs
        if imgs is not None:
            w_img, x_imgs = imgs
            d_img = d_img_in                                                   # e.g. the LSTM backward already made it
            if d_img is None and fuse_act:
                d_img = Bf16Image.empty_rows(N, rowmap, w_img.fmt, dy.device)
                L.check(L.op16("ft_bf16_image_rows_act_bwd_acc", w_img.fmt)(L.ptr(dy), N, L.ptr(y), N, ctx.act, d_img.rows, N, L.ptr(d_img.buf),
                                                                             L.ptr(d_img.colsum), L.ptr(rowmap.map), L.ptr(rowmap.rows), L.stream()),
                        "ft_bf16_image_rows_act_bwd_acc")            # (empty_rows' colsum is a zeroed slab slice)
            elif d_img is None:
                d_img = Bf16Image(dpre.reshape(rows, N), colsum=want_db, mode=w_img.fmt, rowmap=rowmap)   # bias gradient rides on the conversion pass
            db = d_img.colsum if want_db else None
        if want_db and db is None:
            db = colsum(dpre, rows, N, N)
        mrows = rows if rowmap is None else rowmap.cap
        for i, x in enumerate(xs):
            K = x.shape[-1]
            if ctx.needs_input_grad[6 + i]:
                # dx[r,k] = sum_n dpre[r,n] W[n, off+k]
                if imgs is not None:
                    dx, acc = _dx_buffer(x)            # (another consumer of x may have left its contribution there: beta = 1)
                    gemm_img(d_img, 0, d_img.ptr(), w_img, 1, w_img.ptr(0, off), dx, mrows, K, N, K, beta=1.0 if acc else 0.0,
                             rowmap=rowmap, compact=1)
                    if rowmap is not None and "dx" in ctx.fill:
                        rowmap.fill(dx.reshape(rows, K), K, copy_separator=False)
                    if acc:
                        dx = None                      # autograd already holds the buffer through the first consumer
                else:
                    dx = torch.empty_like(x)
                    gemm_raw(dpre, W[:, off:], dx, rows, K, N, N, 1, Ktot, 1, K, mode=ctx.mode_dx)
                dxs.append(dx)
            else:
                dxs.append(None)
            if dW is not None and ctx.cat:
                if i == 0:      # one split-K GEMM over the concatenated image: dW[n, :] = sum_r dpre[r,n] [x_0 | x_1][r, :]
                    weight_grad_gemm(W, dW, d_img, d_img.ptr(), x_imgs[0], x_imgs[0].ptr(), dW, N, Ktot, mrows, Ktot, beta=1.0, rowmap=rowmap, compact=2)
            elif dW is not None:
                # dW[n, off+k] = sum_r dpre[r,n] x[r,k]
                if imgs is not None:
                    weight_grad_gemm(W, dW, d_img, d_img.ptr(), x_imgs[i], x_imgs[i].ptr(), dW[:, off:], N, K, mrows, Ktot, beta=1.0,
                                     rowmap=rowmap, compact=2)
                    if rowmap is not None:
                        _handoff_put_x(x, x_imgs[i])
                else:
                    gemm_raw(dpre, x, dW[:, off:], N, K, rows, 1, N, K, 1, Ktot, mode=ctx.mode_dw, splitk=True)
            off += K
        ctx.imgs = None
        return (dW, db, None, None, None, None, *dxs)


def _linear_images_again(ctx, W, xs, rows):
    """the operand images a LinearFn forward made, made again from the same sources for a second backward through the graph: the
    split [hi] blocks of the encoder convolution (from x itself where the column matrix was never written), the concatenated or
    per-input compact images of the image path"""
    Ktot = W.shape[1]
    if ctx.img_kind == "split3":
        m = ctx.mode_dx
        xi = Bf16Image.split3_im2col(*ctx.lazy_src, m) if ctx.lazy_src is not None else Bf16Image.split3(xs[0].reshape(rows, Ktot), m, False)
        return Bf16Image.of_weight(W, m, split=True).view_cols(Ktot), [xi.view_cols(Ktot)]
    w_img = Bf16Image.of_weight(W, ctx.mode)
    if ctx.cat:
        return w_img, [Bf16Image.cat_rows([x.reshape(rows, x.shape[-1]) for x in xs], ctx.mode, ctx.rowmap)]
    return w_img, [shared_image(x, rows, x.shape[-1], ctx.mode, ctx.rowmap) for x in xs]


_GATE_ON_CAT = True        # the gate layer on the decoder input projection's concatenated image (round 4)


def linear_gate_fusable(mode, rowmap, xs, N):
    """whether LinearGateFn applies: two inputs over a row map on the concatenated-image path (LinearFn's own conditions)"""
    if not (_GATE_ON_CAT and _CAT_IMAGES and rowmap is not None and len(xs) == 2):
        return False
    rows = xs[0].numel() // xs[0].shape[-1]
    return rows == rowmap.T * rowmap.B and linear_uses_images(mode, rows, N, xs)


class LinearGateFn(torch.autograd.Function):
    """y = [x0 | x1] W^T + b  AND  gate = [x0 | x1] wg^T + bg  from ONE concatenated compact image (flowtron.py:758-761: the decoder
    LSTM's input and the gate layer both read [h_att ; ctx]).  The N = 1 gate projection is a GEMV over the image the GEMM has just
    used (ft_img_gemv_rows) instead of two fp32 GEMMs with one output column; in backward its input gradient dgate (x) wg rides on
    the projection's dX GEMMs as a rank-1 epilogue term (no [T,B,1664] fp32 tensor, no accumulation pass) and its weight gradient
    is a GEMV^T over the same image.  Rows of padded frames: y as LinearFn (`fill`), gate = the utterance's separator value."""

    @staticmethod
    def forward(ctx, W, bias, Wg, bg, mode, rowmap, fill, x0, x1):
        xs = [_c(x0), _c(x1)]
        L.require_cuda(W, Wg, *xs)
        W, Wg = _c(W), _c(Wg)
        N, Ktot = W.shape
        assert Wg.shape == (1, Ktot) and xs[0].shape[-1] + xs[1].shape[-1] == Ktot
        rows = rowmap.T * rowmap.B
        c16 = "c16" in fill                       # y as 16-bit rows for a persistent recurrence (gx16_ok)
        y = torch.empty(xs[0].shape[:-1] + (N,), device=W.device, dtype=op16_dtype(mode) if c16 else torch.float32)
        gate = torch.empty(xs[0].shape[:-1] + (1,), device=W.device, dtype=torch.float32)
        w_img = Bf16Image.of_weight(W, mode)
        x_cat = Bf16Image.cat_rows([x.reshape(rows, x.shape[-1]) for x in xs], mode, rowmap)
        gemm_img(x_cat, 0, x_cat.ptr(), w_img, 0, w_img.ptr(), y, rowmap.cap, N, Ktot, N, bias=bias, rowmap=rowmap, compact=1, c16=c16)
        L.check(L.op16("ft_img_gemv_rows", mode)(L.ptr(x_cat.buf), x_cat.ld, Ktot, L.ptr(Wg), L.ptr(bg), L.ptr(gate), 1, L.ptr(rowmap.map),
                                                 L.ptr(rowmap.rows), L.ptr(rowmap.lens), rowmap.T, rowmap.B, L.stream()), "ft_img_gemv_rows")
        if "y" in fill:
            rowmap.fill(y.reshape(rows, N), N, copy_separator=True)
        ctx.save_for_backward(W, Wg, *xs)
        ctx.imgs = (w_img, x_cat)
        ctx.mode, ctx.has_bias, ctx.has_gbias, ctx.rowmap, ctx.fill = mode, bias is not None, bg is not None, rowmap, fill
        return y, gate

    @staticmethod
    def backward(ctx, dy, dgate):
        W, Wg, *xs = ctx.saved_tensors
        N, Ktot = W.shape
        rowmap = ctx.rowmap
        rows = rowmap.T * rowmap.B
        if ctx.imgs is None:                           # (released by a first backward through the graph: retain_graph)
            ctx.imgs = (Bf16Image.of_weight(W, ctx.mode), Bf16Image.cat_rows([x.reshape(rows, x.shape[-1]) for x in xs], ctx.mode, rowmap))
        w_img, x_cat = ctx.imgs
        want_db = ctx.has_bias and ctx.needs_input_grad[1]
        d_img, dy = _dy_image(dy, w_img, rowmap, want_db)
        if d_img is None:
            d_img = Bf16Image(dy.reshape(rows, N), colsum=want_db, mode=w_img.fmt, rowmap=rowmap)
        db = d_img.colsum if want_db else None
        rank1 = None
        if dgate is not None:
            dgate = _c(dgate)
            _require_written(dgate)
        dxs, off = [], 0
        for i, x in enumerate(xs):
            K = x.shape[-1]
            if ctx.needs_input_grad[7 + i]:
                dx, acc = _dx_buffer(x)
                if dgate is not None:
                    rank1 = (dgate, Wg.data_ptr() + 4 * off)
                gemm_img(d_img, 0, d_img.ptr(), w_img, 1, w_img.ptr(0, off), dx, rowmap.cap, K, N, K, beta=1.0 if acc else 0.0,
                         rowmap=rowmap, compact=1, rank1=rank1)
                if "dx" in ctx.fill:
                    rowmap.fill(dx.reshape(rows, K), K, copy_separator=False)
                dxs.append(None if acc else dx)
            else:
                dxs.append(None)
            off += K
        dW = None
        if ctx.needs_input_grad[0]:
            dW = weight_grad_out(W)
            weight_grad_gemm(W, dW, d_img, d_img.ptr(), x_cat, x_cat.ptr(), dW, N, Ktot, rowmap.cap, Ktot, beta=1.0, rowmap=rowmap, compact=2)
        dWg = dbg = None
        if dgate is not None and (ctx.needs_input_grad[2] or (ctx.has_gbias and ctx.needs_input_grad[3])):
            acc = zeroed((Ktot + 1,), W.device)
            L.check(L.op16("ft_img_gemv_rows_bwd", w_img.fmt)(L.ptr(x_cat.buf), x_cat.ld, Ktot, L.ptr(dgate), 1, L.ptr(acc), acc.data_ptr() + 4 * Ktot,
                                                              L.ptr(rowmap.map), L.ptr(rowmap.rows), rowmap.cap, L.stream()), "ft_img_gemv_rows_bwd")
            dWg = acc[:Ktot].reshape(1, Ktot) if ctx.needs_input_grad[2] else None
            dbg = acc[Ktot:] if (ctx.has_gbias and ctx.needs_input_grad[3]) else None
        elif dgate is None:
            dWg = torch.zeros_like(Wg) if ctx.needs_input_grad[2] else None
            dbg = torch.zeros(1, device=W.device, dtype=torch.float32) if (ctx.has_gbias and ctx.needs_input_grad[3]) else None
        ctx.imgs = None
        return (dW, db, dWg, dbg, None, None, None, *dxs)


def linear(xs, W, bias=None, act=L.ACT_NONE, mode=None, rowmap=None, fill="y+dx"):
    if isinstance(xs, torch.Tensor):
        xs = [xs]
    return LinearFn.apply(W, bias, act, L.mfma_mode() if mode is None else mode, rowmap, fill, *xs)


# --------------------------------------------------------------------------
# embedding gather (flowtron.py:873-874)
# --------------------------------------------------------------------------
class EmbeddingFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ids, W, run_stride=0):
        L.require_cuda(ids, W)
        ids = _c(ids.reshape(-1).to(torch.int64))
        W = _c(W)
        out = torch.empty(ids.numel(), W.shape[1], device=W.device, dtype=torch.float32)
        L.check(L.lib().ft_embedding_fwd(L.ptr(ids), L.ptr(W), L.ptr(out), ids.numel(), W.shape[1], W.shape[1], L.stream()),
                "ft_embedding_fwd")
        ctx.save_for_backward(ids, W)
        ctx.run_stride = int(run_stride)
        return out

    @staticmethod
    def backward(ctx, dout):
        ids, W = ctx.saved_tensors
        dout = _c(dout)
        _dw_other_gradient(W)
        dW = weight_grad_out(W)                     # zero-filled; the scatter-add accumulates
        if ctx.run_stride > 0:
            L.check(L.lib().ft_embedding_bwd_runs(L.ptr(ids), L.ptr(dout), L.ptr(dW), ids.numel(), W.shape[1], W.shape[1], ctx.run_stride,
                                                  L.stream()), "ft_embedding_bwd_runs")
        else:
            L.check(L.lib().ft_embedding_bwd(L.ptr(ids), L.ptr(dout), L.ptr(dW), ids.numel(), W.shape[1], W.shape[1], L.stream()),
                    "ft_embedding_bwd")
        return None, dW, None


def embedding(ids, W, run_stride=0):
    """run_stride > 0: the ids repeat with this period (row r carries ids[r % run_stride]'s value in practice) -- the backward then
    sums runs in registers (ft_embedding_bwd_runs); any ids are handled correctly"""
    return EmbeddingFn.apply(ids, W, run_stride)


# --------------------------------------------------------------------------
# encoder conv as im2col + GEMM, masked instance norm + relu (+dropout mask)
# --------------------------------------------------------------------------
# Im2colFn outputs whose VALUES have not been written (lazy = True): data_ptr -> (x, lens, KW).  conv_norm_relu passes such a matrix
# straight to the split-image Linear, whose forward makes the operand image from x itself (Bf16Image.split3_im2col) and whose backward
# reads only that image; any other reader must call _materialize_col first.
_LAZY_COLS = {}


def _materialize_col(col):
    src = _LAZY_COLS.pop(col.data_ptr(), None)
    if src is not None:
        x, lens, KW = src
        Lx, B, Cc = x.shape
        L.check(L.lib().ft_im2col(L.ptr(x), L.ptr(col), L.ptr(lens), Lx, B, Cc, KW, L.stream()), "ft_im2col")


class Im2colFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lens, KW, lazy=False):
        x = _c(x)
        L.require_cuda(x, lens)
        Lx, B, Cc = x.shape
        col = torch.empty(Lx, B, Cc * KW, device=x.device, dtype=torch.float32)
        if lazy:
            _LAZY_COLS[col.data_ptr()] = (x, lens, KW)
        else:
            L.check(L.lib().ft_im2col(L.ptr(x), L.ptr(col), L.ptr(lens), Lx, B, Cc, KW, L.stream()), "ft_im2col")
        ctx.save_for_backward(lens)
        ctx.dims = (Lx, B, Cc, KW)
        return col

    @staticmethod
    def backward(ctx, dcol):
        (lens,) = ctx.saved_tensors
        Lx, B, Cc, KW = ctx.dims
        dcol = _c(dcol)
        dx = torch.empty(Lx, B, Cc, device=dcol.device, dtype=torch.float32)
        L.check(L.lib().ft_col2im(L.ptr(dcol), L.ptr(dx), L.ptr(lens), Lx, B, Cc, KW, L.stream()), "ft_col2im")
        return dx, None, None, None


class InstNormReluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, keep, lens, eps):
        x, gamma, beta = _c(x), _c(gamma), _c(beta)
        L.require_cuda(x, gamma, beta, keep, lens)
        if keep is not None:
            keep = _c(keep)
        Lx, B, Cc = x.shape
        y = torch.empty_like(x)
        mean = torch.empty(B, Cc, device=x.device, dtype=torch.float32)
        rstd = torch.empty_like(mean)
        L.check(L.lib().ft_instnorm_relu_fwd(L.ptr(x), L.ptr(gamma), L.ptr(beta), L.ptr(keep), L.ptr(lens), L.ptr(y),
                                             L.ptr(mean), L.ptr(rstd), Lx, B, Cc, eps, L.stream()), "ft_instnorm_relu_fwd")
        ctx.save_for_backward(x, y, gamma, keep, lens, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, gamma, keep, lens, mean, rstd = ctx.saved_tensors
        dy = _c(dy)
        Lx, B, Cc = x.shape
        dx = torch.empty_like(x)
        dg = torch.empty_like(gamma)
        db = torch.empty_like(gamma)
        L.check(L.lib().ft_instnorm_relu_bwd(L.ptr(x), L.ptr(y), L.ptr(dy), L.ptr(gamma), L.ptr(keep), L.ptr(lens),
                                             L.ptr(mean), L.ptr(rstd), L.ptr(dx), L.ptr(dg), L.ptr(db), Lx, B, Cc, L.stream()),
                "ft_instnorm_relu_bwd")
        return dx, dg, db, None, None, None


def conv_norm_relu(x, lens, conv_w, conv_b, gamma, beta, keep=None, eps=1e-5, mode=None):
    """x [L,B,C] -> relu(masked_instance_norm(conv1d_k5(x))) * keep  (flowtron.py:499-502)."""
    Cout, Cin, KW = conv_w.shape
    # split-image forward (model.Encoder's default in the 16-bit modes): the column matrix is needed as an operand image only -- made from
    # x itself; the fp32 matrix stays unwritten (Im2colFn lazy) unless the Linear cannot take the image path after all
    rows, K = x.shape[0] * x.shape[1], Cin * KW
    lazy = (isinstance(mode, tuple) and mode[0] == "split3" and L.is16(mode[1]) and mode[1] == mode[2] and K % 32 == 0
            and images_apply(mode[1], rows, Cout, K))
    col = Im2colFn.apply(x, lens, KW, lazy)
    y = linear(col, conv_w.reshape(Cout, Cin * KW), conv_b, mode=mode)
    if lazy:
        _materialize_col(col)                    # (a no-op when the Linear took the image from x: it popped the entry)
    return InstNormReluFn.apply(y, gamma, beta, keep, lens, eps)


# --------------------------------------------------------------------------
# length-masked LSTM sequence (packed nn.LSTM semantics, flowtron.py:689-694, :505-512)
# --------------------------------------------------------------------------
# --------------------------------------------------------------------------
# persistent recurrence kernels (csrc/lstm_persist.hip): one launch per sequence, W_hh resident in registers
# --------------------------------------------------------------------------
# The kernels raise a device status word instead of hanging when their hand-off waits time out (grid not co-resident,
# partitioned device, a foreign kernel holding CUs).  Nothing here stalls the stream and nothing kills a run:
#   * a self-test on first use (synchronous, once per device) decides whether the path is usable at all;
#   * afterwards every launch first looks at an asynchronous host copy of the word made after the PREVIOUS launch: a failure
#     surfaces one launch late, is logged ONCE, and switches this device to the launch-per-step kernels for good;
#   * the step that contained the failed launch never reaches the weights: the word stays set until the optimizer (or the DP
#     wrapper, before the gradient all-reduce) has enqueued `if (status) grad[0] = NaN` (ft_poison_if_nonzero), and the fused
#     RAdam kernel drops an update whose global gradient norm is not finite (ft_radam_step) -- on every rank, without a host
#     synchronisation.  While the word is set, further persistent launches of that step abort at their first wait.
_PERSIST = {}


class _PersistState:
    def __init__(self, device):
        self.status = torch.zeros(1, device=device, dtype=torch.int32)
        self.host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self.event = None
        self.usable = None          # None = not tested yet
        self.fail_seen = False      # the host has noticed a failure whose status word has not been consumed (poisoned) yet
        self.failures = 0


def _persist_state(device):
    st = _PERSIST.get(device)
    if st is None:
        st = _PERSIST[device] = _PersistState(device)
    return st


def persist_status(device):
    return _persist_state(device).status


def _persist_failed(st, device, code, where):
    import warnings
    st.usable = False
    st.fail_seen = True
    st.failures += 1
    st.event = None
    warnings.warn("flowtron_amd: a persistent recurrence launch on %s did not complete (status %d, seen %s): the 256-workgroup grid was "
                  "not co-resident / the XCD census failed.  That optimizer step is dropped (non-finite-norm guard) and this device "
                  "uses the launch-per-step kernels from now on." % (device, code, where))


def _persist_watch(device):
    """look at the asynchronous host copy of the status word made after the previous persistent launch (no stall)"""
    st = _persist_state(device)
    if st.event is not None and st.event.query():
        code = int(st.host[0])
        st.event = None
        if code != 0 and not st.fail_seen:
            _persist_failed(st, device, code, "one launch late")
    return st


def persist_consume_failure(device):
    """Called by whoever has just enqueued the poison of this step's gradients (optim.poison_from_status): once the host has seen
    the failure, the status word is cleared BEHIND the poison kernel on the stream, so exactly the affected steps are dropped."""
    st = _PERSIST.get(device)
    if st is not None and st.fail_seen:
        st.status.zero_()
        st.fail_seen = False


PERSIST_LAUNCHES = 0          # persistent (whole-chip, co-resident) kernel launches so far: dist.py keeps collectives away from them


BILSTM_PERSIST_LAUNCHES = 0   # launches of the encoder's persistent bidirectional kernels (csrc/bilstm_persist.hip)


def _persist_arm(st, bilstm=False):
    global PERSIST_LAUNCHES, BILSTM_PERSIST_LAUNCHES
    if bilstm:
        BILSTM_PERSIST_LAUNCHES += 1
    else:
        PERSIST_LAUNCHES += 1
    if st.event is not None:
        # the previous asynchronous copy has not been looked at yet (the host runs about a step ahead of the device): one copy in
        # flight is enough -- the word stays set until it is consumed, so the next copy sees a failure of any launch before it --
        # and a D2H copy per launch costs the stream ~10 us each (copy dispatch + the gap behind it; profiles/r04_v1_step_timeline.txt)
        return
    st.host.copy_(st.status, non_blocking=True)
    st.event = torch.cuda.Event()
    st.event.record()


def check_persist_status(raise_on_failure=True):
    """Host check (one sync) of every persistent-kernel status word.  Tests / bench / inference call it where a garbage result
    must not go unnoticed; returns True when everything completed.  On a failure the device is switched to the launch-per-step
    kernels; with raise_on_failure the caller gets a RuntimeError (the result it just computed is invalid), otherwise False
    (the caller re-runs, e.g. AR_Step.infer on the staged decode chain)."""
    ok = True
    for dev, st in _PERSIST.items():
        code = int(st.status.item())
        if code != 0:
            ok = False
            if not st.fail_seen:
                _persist_failed(st, dev, code, "by a synchronous check")
            st.status.zero_()
            st.fail_seen = False
            if raise_on_failure:
                raise RuntimeError("persistent kernel timed out on %s (status %d): the 256-workgroup grid was not co-resident; the "
                                   "launch-per-step kernels are used from now on (FLOWTRON_LSTM_PERSIST=0 selects them up front)" % (dev, code))
    return ok


PERSIST_BWD_CODE = 21        # ft_lstm_persist_bwd's one transport: the reduce-scatter kernel (csrc/lstm_persist.hip)


def _persist_bwd(dy, w_hh, lens, gates, cell, dgx, d_img, mode):
    """ONE launch of the reduce-scatter backward recurrence (csrc/lstm_persist.hip; B <= 32) over contiguous [T, B, .] tensors: dgates as
    fp32 rows into `dgx`, as compact 16-bit image + column sums into `d_img` (over T B + B rows), or both -- one of the two may be None"""
    T, B, H = cell.shape
    st = _persist_watch(dy.device)
    work = torch.empty(L.lib().ft_lstm_persist_workspace_bytes(B, H), device=dy.device, dtype=torch.uint8)
    args = (L.ptr(dy), H, L.ptr(w_hh), L.ptr(lens), L.ptr(gates), L.ptr(cell), L.ptr(dgx), L.ptr(work), L.ptr(st.status), T, B, H, PERSIST_BWD_CODE)
    if d_img is None:
        L.check(L.op16("ft_lstm_persist_bwd", mode)(*args, L.stream()), "ft_lstm_persist_bwd")
    else:
        L.check(L.op16("ft_lstm_persist_bwd_img", mode)(*args, L.ptr(d_img.buf), d_img.ld, d_img.buf.numel() // (2 * d_img.ld), L.ptr(d_img.colsum),
                                                        L.stream()), "ft_lstm_persist_bwd_img")
    _persist_arm(st)


def _persist_selftest(device):
    """tiny forward + backward through the persistent kernels the TRAINING step launches -- the roles forward at 4 and at 8 rows per
    XCD group with two roles (csrc/lstm_roles.hip: its own launch context and LDS sizes), the reduce-scatter backward once through
    ft_lstm_persist_bwd and once through the image-only entry the step itself uses (ft_lstm_persist_bwd_img) -- checked
    synchronously, once per device (a device where only some of the kernels are co-resident must not pass the self-test
    and then drop its first optimizer steps)."""
    H, B, T = 1024, 8, 3
    f = dict(device=device, dtype=torch.float32)
    gx, w = torch.zeros(T, B, 4 * H, **f), torch.zeros(4 * H, H, **f)
    lens = torch.full((B,), T, dtype=torch.int32, device=device)
    y, gates, cell = torch.empty(T, B, H, **f), torch.empty(T, B, 4 * H, **f), torch.empty(T, B, H, **f)
    dgx = torch.empty(T, B, 4 * H, **f)
    st = _persist_state(y.device)        # (the state the launches report to: a `device` without an index names the same card)
    try:
        wimg = roles_wimg(w, L.FT_BF16, False)
        roles_launch([fwd_role(gx, lens, y, gates, cell, wimg)], 4, L.FT_BF16, device)
        roles_launch([fwd_role(gx, lens, y, gates, cell, wimg), fwd_role(gx, lens, y, gates, cell, wimg)], 8, L.FT_BF16, device)
        _persist_bwd(y, w, lens, gates, cell, dgx, None, L.FT_BF16)
        if _PERSIST_IMG != "0":
            dimg = Bf16Image._blank(T * B + B, 4 * H, L.FT_BF16, device)
            dimg.colsum = torch.zeros(4 * H, **f)
            _persist_bwd(y, w, lens, gates, cell, None, dimg, L.FT_BF16)
        ok = int(st.status.item()) == 0
    except RuntimeError:
        ok = False
    st.status.zero_()
    st.event = None
    if not ok:
        import warnings
        warnings.warn("flowtron_amd: the persistent LSTM kernels are not usable on %s (grid not co-resident / XCD census failed); "
                      "using the launch-per-step kernels" % (device,))
    return ok


def _persist_env():
    """FLOWTRON_LSTM_PERSIST: 1 (default), or 0 = the launch-per-step kernels (the yardstick path of the tests).  Read per call."""
    v = int(_os.environ.get("FLOWTRON_LSTM_PERSIST", "1"))
    if v not in (0, 1):
        raise ValueError("FLOWTRON_LSTM_PERSIST must be 0 or 1 (the transport variants were removed in round 6)")
    return v


def _persist_passed(device):
    """the self-test's verdict on this device: made at the first question, withdrawn for good by a launch that fails (_persist_failed)"""
    st = _persist_state(device)
    if st.usable is None:
        st.usable = _persist_selftest(device)
    return bool(st.usable)


def persist_usable(device):
    """True if the persistent kernels passed their self-test on this device.  FLOWTRON_LSTM_PERSIST is NOT consulted: it switches the
    training recurrences, and the decode path, which asks here, has a switch of its own (FLOWTRON_DECODE_PERSIST)."""
    return bool(L.lib().ft_lstm_persist_supported(8, 1024)) and _persist_passed(torch.device(device))


def lstm_persist_groups(B, H, reverse, mode, device=None):
    """1 when the persistent recurrence kernels take this shape in one launch per sequence (H 1024, B <= 32, forward direction,
    16-bit operands, a device that passed the self-test), else 0 = the launch-per-step kernels.  FLOWTRON_LSTM_PERSIST=0 switches
    the persistent kernels off."""
    return int(bool(_persist_env() and not reverse and L.is16(mode) and L.lib().ft_lstm_persist_supported(B, H)
                    and (device is None or _persist_passed(device))))


def lstm_persistent(B, H, reverse, mode, device):
    """whether a persistent recurrence runs a layer of this shape: in one launch up to B 32, in slices of a wider batch (roles_plan)"""
    return bool(lstm_persist_groups(min(B, 32), H, reverse, mode, device))


def lstm_persist_slices(B, H, reverse, mode, device=None):
    """True for a batch wider than the 4-row kernels hold (B > 32) where the roles kernels apply: 8 rows per XCD group up to B 64, 16
    up to 128 per launch forward / slices of 64 backward (roles_plan; 1.93 us per step at B 64 against 2 x 1.76 for two sliced launches
    of the round-5 kernel, 6.8 us for the launch-per-step kernels at B 48).  False: one launch suffices, or the shape is not theirs."""
    return B > 32 and lstm_persistent(B, H, reverse, mode, device)


# b_ih + b_hh of the LSTMs of a flow (and of the encoder) in ONE launch each per forward (a multi-tensor add; eight elementwise launches
# of ~5 us stood there: VERDICT r5 weak #12).  model.Flowtron.forward brackets its pass with bias_sums_begin / bias_sums_end; outside such a
# bracket -- and for a pair the bracket did not list -- bias_sum is the plain add.
_BIAS_SUMS = {}


class _BiasSumsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *flat):
        n = len(flat) // 2
        return tuple(torch._foreach_add(list(flat[:n]), list(flat[n:])))

    @staticmethod
    def backward(ctx, *gs):
        return tuple(gs) + tuple(gs)


def bias_sums_begin(groups):
    """groups: lists of (b_ih, b_hh) pairs; one launch (and one autograd node) per group, made at the group's FIRST request -- the
    node then sits where the first of the adds it replaces sat, and backward reaches it in the same order"""
    _BIAS_SUMS.clear()
    for pairs in groups:
        pairs = [(a, b) for a, b in pairs if a.is_cuda and b.is_cuda and a.shape == b.shape]
        if len(pairs) < 2:
            continue
        group = {"pairs": pairs, "outs": None}
        for a, b in pairs:
            _BIAS_SUMS[(id(a), id(b))] = group


def bias_sums_end():
    _BIAS_SUMS.clear()


def bias_sum(a, b):
    g = _BIAS_SUMS.get((id(a), id(b)))
    if g is None:
        return a + b
    if g["outs"] is None:
        g["outs"] = _BiasSumsFn.apply(*[x for x, _ in g["pairs"]], *[y for _, y in g["pairs"]])
    for (x, y), o in zip(g["pairs"], g["outs"]):
        if x is a and y is b:
            return o
    return a + b


PERSIST_H = 1024                  # the hidden size the persistent recurrence kernels are built for
_PAD_H = True    # hidden sizes below it on the persistent kernels through zero-padded gate blocks (tests set it False: the yardstick)


def lstm_pad_width(B, H, reverse, mode, device, T):
    """True where a layer with H < 1024 hidden units should run as its zero-padded 1024-unit twin (lstm_layer): the persistent kernels
    take the padded shape and the sequence is long enough for 1.3-1.6 us per step against the launch-per-step kernels' 5-6 to pay for the
    wider projection (4096 gate columns instead of 4 H)"""
    if not _PAD_H or H >= PERSIST_H or H < 256 or H % 8 or reverse or T < 64:      # (H < 256: > 4 x the gate columns and saved gates)
        return False
    return lstm_persistent(B, PERSIST_H, reverse, mode, device)


def pad_gate_blocks(w, pad_cols):
    """[4 H, X] (or [4 H]) -> [4 * 1024, X + pad_cols]: each of the four gate blocks zero-padded to 1024 rows, X to X + pad_cols columns"""
    H = w.shape[0] // 4
    if w.dim() == 1:
        return torch.nn.functional.pad(w.view(4, H), (0, PERSIST_H - H)).reshape(4 * PERSIST_H)
    return torch.nn.functional.pad(w.view(4, H, w.shape[1]), (0, pad_cols, 0, PERSIST_H - H)).reshape(4 * PERSIST_H, w.shape[1] + pad_cols)


def bilstm_persist_ok(B, H, mode, device):
    """the encoder-shaped persistent bidirectional kernels (H 256, B <= 32, 16-bit operands) on a device whose persistent grids
    passed the self-test; FLOWTRON_LSTM_PERSIST=0 keeps the launch-per-step pair chain"""
    return bool(_persist_env() and L.is16(mode) and L.lib().ft_bilstm_persist_supported(B, H) and _persist_passed(device))


# ---- round 6: rows per XCD group / time windows / two roles per launch (csrc/lstm_roles.hip) ------------------------------------
class RolesCtx:
    """Launch context of the ft_lstm_roles_* kernels on one device: hand-off sets + census counters (initialised once) and the
    launch counters of the two kernel kinds (a launch works in set phase & 1 and presets the other one for its successor)."""

    def __init__(self, device):
        self.buf = torch.empty(L.lib().ft_lstm_roles_ctx_bytes(), device=device, dtype=torch.uint8)
        L.check(L.lib().ft_lstm_roles_ctx_init(L.ptr(self.buf), L.stream()), "ft_lstm_roles_ctx_init")
        self.phase = [0, 0]          # forward, backward
        self.reset_rows = 8          # the largest R any later launch of a kind may use (roles_reset_rows)


_ROLES_CTX = {}


def roles_ctx(device):
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    c = _ROLES_CTX.get(device)
    if c is None:
        c = _ROLES_CTX[device] = RolesCtx(device)
    return c


WFRAG_TABLE_MAX = 16


def _wfrag_planned(w_hh, mode, backward):
    """roles_wimg inside the weight-image plan of a model (weight_images_begin): the image of a planned weight, made with all the others
    in ONE launch at the forward's first request (ft_lstm_roles_prepare_table), or None.  A forward request of a parameter enters the
    plan of the NEXT forward; a backward request marks its entry, so that the next forward with gradients enabled also makes the backward
    image (gradient mode as weight_images_begin found it; it waits in the cache until the backward takes it, or until the next forward begins; taken only while the weight's version
    is the one it was made from).  Every forward builds from the current values: nothing is kept from step to step."""
    w = _WIMG
    key = (w_hh.data_ptr(), tuple(w_hh.shape), mode)
    if backward:
        e = w["wf_last"].get(key) if w["wf_last"] is not None else None
        if e is not None:
            e[1] = True
    elif w["wf_plan_next"] is not None and isinstance(w_hh, torch.nn.Parameter) and w_hh.shape[1] == PERSIST_H:
        prev = w["wf_plan"].get(key)
        w["wf_plan_next"][key] = [w_hh, bool(prev is not None and prev[1])]
    if w["wf_armed"] and not backward:
        w["wf_armed"] = False
        nbytes = L.lib().ft_lstm_roles_wimg_bytes(PERSIST_H)
        plan = [(k, t, bw) for k, (t, bw) in w["wf_plan"].items() if t.is_cuda and t.device == w_hh.device and t.dtype == torch.float32
                and t.is_contiguous() and t.data_ptr() == k[0] and tuple(t.shape) == k[1]]
        for fmt in sorted({k[2] for k, _, _ in plan}):
            items = [p for p in plan if p[0][2] == fmt]
            for lo in range(0, len(items), WFRAG_TABLE_MAX):
                part = items[lo:lo + WFRAG_TABLE_MAX]
                descs = (L.WfragDesc * len(part))()
                for i, (k, t, bw) in enumerate(part):
                    f_img = torch.empty(nbytes, device=t.device, dtype=torch.uint8)
                    b_img = torch.empty(nbytes, device=t.device, dtype=torch.uint8) if bw and w["wf_grad"] else None
                    descs[i] = L.WfragDesc(t.data_ptr(), L.ptr(f_img), L.ptr(b_img))
                    w["wf_cache"][(k, False)] = (f_img, t, t._version)
                    if b_img is not None:
                        w["wf_cache"][(k, True)] = (b_img, t, t._version)
                L.check(L.op16("ft_lstm_roles_prepare_table", fmt)(descs, len(part), PERSIST_H, L.stream()), "ft_lstm_roles_prepare_table")
    hit = w["wf_cache"].pop((key, bool(backward)), None)
    if hit is not None and hit[2] == w_hh._version:          # (same storage by the key; unchanged since the table read it)
        return hit[0]
    return None


def roles_wimg(w_hh, mode, backward):
    """MFMA fragment image of W_hh for the roles kernels (forward: gate-adjacent tiles; backward: the reduce-scatter layout)."""
    if _WIMG_ON:
        img = _wfrag_planned(w_hh, mode, backward)
        if img is not None:
            return img
    img = torch.empty(L.lib().ft_lstm_roles_wimg_bytes(w_hh.shape[1]), device=w_hh.device, dtype=torch.uint8)
    fn = L.op16("ft_lstm_roles_prepare_bwd" if backward else "ft_lstm_roles_prepare_fwd", mode)
    w = _c(w_hh)                 # (named: a temporary copy would be recycled by the allocator before the launch reads it)
    L.check(fn(L.ptr(w), L.ptr(img), w.shape[1], L.stream()), "ft_lstm_roles_prepare")
    return img


def fwd_role(gx, lens, y, gates, cell, wimg, t0=0, t1=None, state=None, b0=0, nb=None, xproj=None):
    """one forward recurrence of a roles launch over the batch rows [b0, b0 + nb) of time-major tensors, window [t0, t1).
    xproj = (x image over the RowMap of `lens`, W_ih image, fp32 bias [4H]): gx is None and the kernel's bursts compute their gx slices
    from the images (the whole batch of the map: b0 == 0; R <= 8)"""
    if xproj is not None:
        x_img, w_img, bias = xproj
        assert gx is None and b0 == 0 and x_img.fmt == w_img.fmt and x_img.cols == w_img.cols and bias.dtype == torch.float32
        T, LB = y.shape[0], y.shape[1]
        nb = LB if nb is None else nb
        return L.LstmFwdRole(None, lens.data_ptr(), y.data_ptr(), y.stride(1), L.ptr(gates), L.ptr(cell), L.ptr(wimg),
                             L.ptr(state[0]) if state is not None else None, L.ptr(state[1]) if state is not None else None,
                             nb, LB, t0, T if t1 is None else t1, 0,
                             x_img.ptr(), w_img.ptr(), L.ptr(bias), x_img.ld, w_img.ld, x_img.rows, x_img.cols)
    T, LB, H = gx.shape[0], gx.shape[1], y.shape[2]
    nb = LB - b0 if nb is None else nb
    return L.LstmFwdRole(gx.data_ptr() + gx.element_size() * 4 * H * b0, lens.data_ptr() + 4 * b0, y.data_ptr() + 4 * y.stride(1) * b0, y.stride(1),
                         gates.data_ptr() + 16 * H * b0 if gates is not None else None, cell.data_ptr() + 4 * H * b0 if cell is not None else None,
                         L.ptr(wimg), L.ptr(state[0]) if state is not None else None, L.ptr(state[1]) if state is not None else None,
                         nb, LB, t0, T if t1 is None else t1, int(gx.dtype != torch.float32))


def bwd_role(dy, lens, gates, cell, dgx, wimg, t0=0, t1=None, state=None, carry_in=False, dimg=None, b0=0, nb=None):
    T, LB, H = gates.shape[0], gates.shape[1], cell.shape[2]
    nb = LB - b0 if nb is None else nb
    return L.LstmBwdRole(dy.data_ptr() + 4 * dy.stride(1) * b0, dy.stride(1), lens.data_ptr() + 4 * b0, gates.data_ptr() + 16 * H * b0,
                         cell.data_ptr() + 4 * H * b0, dgx.data_ptr() + 16 * H * b0 if dgx is not None else None, L.ptr(wimg),
                         L.ptr(dimg.buf) if dimg is not None else None, dimg.ld if dimg is not None else 0,
                         dimg.buf.numel() // (2 * dimg.ld) if dimg is not None else 0, L.ptr(dimg.colsum) if dimg is not None else None,
                         L.ptr(state[0]) if state is not None else None, L.ptr(state[1]) if state is not None else None,
                         nb, LB, t0, T if t1 is None else t1, int(bool(carry_in)))


def roles_launch(roles, R, mode, device, backward=False, H=1024):
    """one launch of lstm_roles_fwd_k / _bwd_k: `roles` = one or two role structs; R rows per XCD group.  Nothing happens when every
    window is empty: the C entries refuse such a call (FT_EINVAL), and a launch counted in `phase` that never ran would leave the next
    one in the wrong hand-off set."""
    if all(r.t1 <= r.t0 for r in roles):
        return
    c = roles_ctx(device)
    if R > c.reset_rows:
        # wider groups than any launch on this context has preset for: start over with the sets preset for R rows (rare: the first
        # batch wider than 64 on a device)
        L.check(L.lib().ft_lstm_roles_ctx_init(L.ptr(c.buf), L.stream()), "ft_lstm_roles_ctx_init")
        c.phase, c.reset_rows = [0, 0], R
    st = _persist_watch(c.buf.device)
    k = 1 if backward else 0
    arr = ((L.LstmBwdRole if backward else L.LstmFwdRole) * len(roles))(*roles)
    fn = L.op16("ft_lstm_roles_bwd" if backward else "ft_lstm_roles_fwd", mode)
    L.check(fn(arr, len(roles), R, c.reset_rows, L.ptr(c.buf), c.phase[k], L.ptr(st.status), H, L.stream()), "ft_lstm_roles")
    c.phase[k] += 1
    _persist_arm(st)


def roles_plan(B, backward):
    """[(first row, rows, rows per XCD group)] of the roles launches that cover a batch of B rows"""
    cap = 64 if backward else 128
    out = []
    for b0 in range(0, B, cap):
        nb = min(cap, B - b0)
        out.append((b0, nb, 4 if nb <= 32 else 8 if nb <= 64 else 16))
    return out


_PAIR_CHUNKS_BWD = int(_os.environ.get("FLOWTRON_LSTM_PAIR_BWD", "3"))   # windows of the pair's BACKWARD pipeline (_pair_backward_pipeline); 0 = the sequential form, -1 = as forward
_PAIR_CHUNKS = int(_os.environ.get("FLOWTRON_LSTM_PAIR", "6"))       # time chunks of the decoder layer pair pipeline; 0 = one recurrence per launch


def decoder_pair_chunks(B, H, mode, device, T):
    """number of time chunks the two decoder layers are pipelined over (DecoderPairFn), or 0: the pair needs both recurrences on
    R = 8 rows per XCD, four XCDs each (B <= 32), the persistent kernels' shape (hence 16-bit operands), a sequence long enough to chunk
    and the compact operand images its backward works on throughout (DecoderPairFn.forward states the same)"""
    if (_PAIR_CHUNKS <= 0 or B > 32 or T < 4 * _PAIR_CHUNKS or not lstm_persist_groups(B, H, False, mode, device)
            or not images_apply(mode, 4 * H, H, (T - 1) * B)):
        return 0
    return _PAIR_CHUNKS


def decoder_plan(n_layers, has_gate, has_rowmap, persistent, pair_chunks, lstm2_ok):
    """(path, fuse_gate) of a flow's decoder LSTM stack (model.AR_Step.forward) from plain values: persistent = lstm_persistent or the
    padded twin (lstm_pad_width), pair_chunks = decoder_pair_chunks.  path: "layers" = any depth but two, layer after layer; "pair" =
    DecoderPairFn; "persistent" / "step" = two single layers; "lstm2" = LSTM2SeqFn, which alone makes layer 0's input projection
    itself: everywhere else the gate layer rides on that projection (fuse_gate)."""
    if n_layers != 2:
        path = "layers"
    elif persistent:
        path = "pair" if has_rowmap and pair_chunks else "persistent"
    else:
        path = "lstm2" if lstm2_ok else "step"
    return path, bool(has_gate and path != "lstm2")


def _chunk_edges(T, n):
    return [(k * T + n // 2) // n for k in range(n + 1)]


_EDGE_CACHE = {}


def _chunk_rowmaps(lens, edges, B):
    """per time chunk [e_k, e_k+1): the chunk as a padded batch of its own -- lengths clamp(len - e_k, 0, width) -- and its RowMap
    (the edge vectors are made on the device once per (edges, device): no host-to-device copy in a step)"""
    key = (tuple(edges), lens.device)
    ev = _EDGE_CACHE.get(key)
    if ev is None:
        T, n = edges[-1], len(edges) - 1
        k = torch.arange(n + 1, device=lens.device, dtype=torch.int64)
        e = torch.div(k * T + n // 2, n, rounding_mode="floor").to(torch.int32)
        if len(_EDGE_CACHE) > 64:
            _EDGE_CACHE.clear()                  # (drops the last-maps entries too)
        ev = _EDGE_CACHE[key] = (e[:-1].contiguous(), (e[1:] - e[:-1]).contiguous())
    # both flows of a forward pass chunk the same lengths the same way: the maps of the last (lens tensor, edges) are kept
    ck = (lens.data_ptr(), lens._version, key)
    if _EDGE_CACHE.get("last_key") == ck and _EDGE_CACHE["last_lens"]() is lens:
        return _EDGE_CACHE["last_maps"]
    lk = torch.minimum((lens[None, :] - ev[0][:, None]).clamp_(min=0), ev[1][:, None])
    maps = [RowMap(lk[k], edges[k + 1] - edges[k], B) for k in range(len(edges) - 1)]
    _EDGE_CACHE["last_key"], _EDGE_CACHE["last_lens"], _EDGE_CACHE["last_maps"] = ck, _weakref.ref(lens), maps
    return maps


def _gather_gemm_on():
    """ft_gemm_img's row gather lives in the 64-wide single-buffer kernel alone: under the library's A/B hooks that switch that kernel off
    (FT_GEMM_BF16_WIDE=0, FT_GEMM_BF16_TILE=256; read per call there, so per call here) the pair's backward takes the sequential form,
    whose one dX GEMM gathers nothing"""
    def num(name, default):
        try:
            return int(_os.environ.get(name, default))
        except ValueError:
            return 0                             # (atoi)
    return num("FT_GEMM_BF16_WIDE", "1") != 0 and num("FT_GEMM_BF16_TILE", "0") != 256


def _chunk_gathers(maps, lens, edges):
    """the chunks' row lists into the whole sequence's batch-major image (ChunkGather; one small launch per chunk), made at the first
    backward that asks for them (the forward's maps need none unless the backward runs over the same chunks): they ride with the maps,
    so both flows, and every step that chunks the same `lens` tensor, make them once"""
    for k, m in enumerate(maps):
        if getattr(m, "gather", None) is None:
            m.gather = ChunkGather(lens, m, edges[-1], edges[k], edges[k + 1])
    return [m.gather for m in maps]


class ChunkGather:
    """Row lists of one time chunk [t0, t1) for a GEMM over the chunk's compact rows that reads them out of the WHOLE sequence's batch-major
    compact image (csrc: ft_chunk_gather_rows): a_rows[i] = the image row of the chunk's compact row i, map[i] = its row in the chunk's
    time-major output -- the chunk RowMap's, with the chunk's separator rows dropped (-1): they read a valid row, because the image's own
    separator rows are only written by the window that holds step 0.  rows / cap are the chunk map's (gemm_img takes this as its rowmap)."""
    __slots__ = ("cap", "map", "rows", "a_rows")

    def __init__(self, lens32, chunk_map, T, t0, t1):
        self.cap, self.rows = chunk_map.cap, chunk_map.rows
        both = torch.empty(2, self.cap, device=lens32.device, dtype=torch.int32)
        self.a_rows, self.map = both[0], both[1]
        L.check(L.lib().ft_chunk_gather_rows(L.ptr(lens32), L.ptr(self.a_rows), L.ptr(self.map), int(T), chunk_map.B, int(t0), int(t1), L.stream()),
                "ft_chunk_gather_rows")


class DecoderPairFn(torch.autograd.Function):
    """Both decoder LSTM layers of a flow (nn.LSTM(.., num_layers=2), flowtron.py:654-655, 689-694) as ONE pipeline over n time chunks:
    launch k runs layer 0 on chunk k (XCDs 0-3, 8 batch rows each) and layer 1 on chunk k - 1 (XCDs 4-7) CONCURRENTLY
    (csrc/lstm_roles.hip: two roles per launch, carried state), and layer 1's input projection of chunk k -- a chip-filling GEMM
    over the chunk's valid rows -- runs between launch k and launch k + 1.  The dependency chain of the pair is (1 + 1/n) T steps of the
    8-row kernel instead of 2 T steps of the 4-row one; the arithmetic is that of two single launches (forward bit-identical).
    Backward has two forms, both over the compact 16-bit dgates images of the whole sequence: the same pipeline the other way round
    (_pair_backward_pipeline, the default: layer 1 on window c, layer 0 on window c + 1, the window's dX GEMM dy0 = dgates1 W_ih1 in
    between, over FLOWTRON_LSTM_PAIR_BWD windows of its own), or two single recurrences around one dX GEMM (_pair_backward_sequential).
    FLOWTRON_LSTM_PERSIST_IMG decides only how layer 0's dgates LEAVE the node (_pair_backward_return).
    The node takes what model.Flowtron gives it where decoder_pair_chunks says yes, and nothing else: a RowMap over its own [T, B],
    16-bit operands, T > 1 and a shape whose weight-gradient GEMMs run from images -- ValueError otherwise, there is no other path."""

    @staticmethod
    def forward(ctx, gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens, mode, rowmap, gx_private, nchunks):
        gx0, w_hh0, w_ih1, w_hh1 = _c(gx0), _c(w_hh0), _c(w_ih1), _c(w_hh1)
        L.require_cuda(gx0, w_hh0, w_ih1, w_hh1, lens)
        T, B, H4 = gx0.shape
        H = H4 // 4
        if rowmap is None or rowmap.T != T or rowmap.B != B:
            raise ValueError("DecoderPairFn needs a RowMap over its own [T, B] = [%d, %d] (ops.row_map)" % (T, B))
        if not L.is16(mode) or T <= 1 or not images_apply(mode, H4, H, (T - 1) * B):
            raise ValueError("DecoderPairFn needs 16-bit operands, T > 1 and weight-gradient GEMMs large enough for operand images "
                             "(mode %s, T %d, B %d, H %d); ops.decoder_pair_chunks says where the pair applies" % (mode, T, B, H))
        dev = gx0.device
        f = dict(device=dev, dtype=torch.float32)
        y0, g0, c0 = torch.empty(T, B, H, **f), torch.empty(T, B, H4, **f), torch.empty(T, B, H, **f)
        y1, g1, c1 = torch.empty(T, B, H, **f), torch.empty(T, B, H4, **f), torch.empty(T, B, H, **f)
        g16 = gx0.dtype != torch.float32          # 16-bit gx rows (decoder_pair: gx16_ok): layer 1's chunk projections write them too
        gx1 = torch.empty(T, B, H4, device=dev, dtype=gx0.dtype)
        # (carried state: written by a window before the next one reads it -- a group that runs in window k ran in window k - 1)
        st0, st1 = torch.empty(2, B, H, **f), torch.empty(2, B, H, **f)
        wi0, wi1 = roles_wimg(w_hh0, mode, False), roles_wimg(w_hh1, mode, False)
        w_img = Bf16Image.of_weight(w_ih1, mode)
        b1 = bias_sum(b_ih1, b_hh1).detach()
        edges = _chunk_edges(T, nchunks)
        rms = _chunk_rowmaps(lens, edges, B)
        for k in range(nchunks + 1):
            roles = []
            if k < nchunks:
                roles.append(fwd_role(gx0, lens, y0, g0, c0, wi0, edges[k], edges[k + 1], st0))
            if k > 0:
                roles.append(fwd_role(gx1, lens, y1, g1, c1, wi1, edges[k - 1], edges[k], st1))
            roles_launch(roles, 8 if len(roles) == 2 else 4, mode, dev)
            if k < nchunks:
                # layer 1's input projection of chunk k over its valid rows, scattered into gx1[e_k : e_k+1]
                a, b = edges[k], edges[k + 1]
                x_img = Bf16Image(y0[a:b].reshape((b - a) * B, H), mode=mode, rowmap=rms[k])
                gemm_img(x_img, 0, x_img.ptr(), w_img, 0, w_img.ptr(), gx1[a:b], rms[k].cap, H4, H, H4, bias=b1, rowmap=rms[k], compact=1, c16=g16)
        ctx.save_for_backward(w_hh0, w_ih1, w_hh1, lens, y0, g0, c0, y1, g1, c1)
        ctx.mode, ctx.rowmap, ctx.gx_private, ctx.nchunks = mode, rowmap, bool(gx_private), nchunks
        ctx.chunk_maps, ctx.w_img, ctx.gx_dtype = (edges, rms), w_img, gx0.dtype
        return y1

    @staticmethod
    def backward(ctx, dy1):
        saved = ctx.saved_tensors                      # w_hh0, w_ih1, w_hh1, lens, y0, g0, c0, y1, g1, c1
        T = saved[7].shape[0]
        w_img = ctx.w_img if ctx.w_img is not None else Bf16Image.of_weight(saved[1], ctx.mode)     # (released by a first backward: retain_graph)
        ctx.w_img = None
        n = min(_PAIR_CHUNKS_BWD, T) if _PAIR_CHUNKS_BWD >= 0 else ctx.nchunks      # (at most T windows: none is empty, the edges rise strictly)
        keep_f32 = _dgates_exit(ctx.gx_private)[1]      # dgx0 as real fp32 values beside the image, which is the only form inside the node
        if n == 0 or not _gather_gemm_on():
            return _pair_backward_sequential(ctx, saved, _c(dy1), w_img, keep_f32)
        return _pair_backward_pipeline(ctx, saved, _c(dy1), w_img, n, keep_f32)


def _dgates_exit(gx_private):
    """How a persistent backward's dgates leave the node, (hand_image, keep_f32).  hand_image: the compact 16-bit image goes to the input
    projection's backward -- FLOWTRON_LSTM_PERSIST_IMG 1: where gx is that projection's own, both: always, 0: never.  keep_f32: fp32
    rows too -- where no image is handed, with "both", and in anomaly mode, which must find real values in every returned gradient."""
    hand = _PERSIST_IMG != "0" and (gx_private or _PERSIST_IMG == "both")
    return hand, not hand or _PERSIST_IMG == "both" or torch.is_anomaly_enabled()


def _leave_dgates(dgx, d_img, shape, gx_dtype):
    """What a recurrence's backward returns for its gx.  dgx None: the NaN face of the dgates image `d_img` (a foreign reader sees NaN,
    never unwritten memory), the image handed to the input projection's backward as the ONLY form.  Else the fp32 rows `dgx` in gx's
    dtype (16-bit gx rows, gx16_ok, in a pass that keeps fp32 dgates: autograd wants the gradient in gx's dtype, and the hand-off is
    keyed on the tensor it will carry), with `d_img` -- where there is one -- handed over beside them: the projection's backward reads
    the same dgates."""
    if dgx is None:
        dgx = image_only_gradient(shape, d_img.buf.device, gx_dtype)
        _handoff_put_image_only(dgx, d_img)
        return dgx
    if dgx.dtype != gx_dtype:
        dgx = dgx.to(gx_dtype)
    if d_img is not None:
        _handoff_put(dgx, d_img)
    return dgx


def _compact_dw(W, d_img, y_img, dW, shift):
    """dW += dgates^T y over the compact rows of the images' RowMap (split-K); shift 1 for a recurrent weight: dgates_t meets h_{t-1}"""
    rm, H = d_img.rowmap, y_img.cols
    weight_grad_gemm(W, dW, d_img, d_img.ptr(shift), y_img, y_img.ptr(0), dW, d_img.cols, H, rm.cap, H, beta=1.0, rowmap=rm, compact=2, k_shift=shift)


def _pair_weight_grads(ctx, saved, d_img1, d_img0):
    """(dW_hh1, dW_ih1, dW_hh0) of the pair from the compact dgates images of the whole sequence (the one-step shift of a dW_hh = one
    compact row); None where the weight needs no gradient"""
    w_hh0, w_ih1, w_hh1, _, y0, _, _, y1 = saved[:8]
    T, B, H = y1.shape
    rm, need = ctx.rowmap, ctx.needs_input_grad
    y0_img = y_image(y0, T * B, H, ctx.mode, rm) if need[1] or need[2] else None
    y1_img = y_image(y1, T * B, H, ctx.mode, rm) if need[5] else None
    jobs = [(need[5], w_hh1, d_img1, y1_img, 1), (need[2], w_ih1, d_img1, y0_img, 0), (need[1], w_hh0, d_img0, y0_img, 1)]
    outs = [weight_grad_out(w) if on else None for on, w, _, _, _ in jobs]
    for dW, (on, w, d, y, shift) in zip(outs, jobs):
        if on:
            _compact_dw(w, d, y, dW, shift)
    return outs


def _pair_backward_return(ctx, saved, d_img1, d_img0, dgx0):
    """the tail both backward forms share: the weight gradients, and dgx0 as _dgates_exit says it leaves the node -- the image alone
    (dgx0 None), fp32 rows with the image beside them, or fp32 rows alone"""
    dW_hh1, dW_ih1, dW_hh0 = _pair_weight_grads(ctx, saved, d_img1, d_img0)
    T, B, H = saved[7].shape
    dgx0 = _leave_dgates(dgx0, d_img0 if _dgates_exit(ctx.gx_private)[0] else None, (T, B, 4 * H), ctx.gx_dtype)
    db1 = d_img1.colsum
    return dgx0, dW_hh0, dW_ih1, db1, db1, dW_hh1, None, None, None, None, None


def _pair_backward_sequential(ctx, saved, dy1, w_img, keep_f32):
    """DecoderPairFn.backward without the pipeline: layer 1's recurrence, ONE dX GEMM over all valid rows, layer 0's recurrence -- the
    round-5 sequence (4-row kernels, dgates of both layers as compact images; keep_f32: layer 0's as fp32 rows beside its image).  The
    backward kernel at 8 rows per group and two roles runs 2.55 us per step against 2 x 1.62, and the chunked dX GEMMs (N = 1024,
    K = 4096: 224 tiles of a chunk) cost 3 x the one GEMM; the pipeline over one dgates image (_pair_backward_pipeline) is still faster
    than this form and is the default -- this one serves FLOWTRON_LSTM_PAIR_BWD=0, and the library's A/B hooks that switch the
    gathering GEMM kernel off (_gather_gemm_on)."""
    w_hh0, w_ih1, w_hh1, lens, y0, g0, c0, y1, g1, c1 = saved
    T, B, H = y1.shape
    H4, mode, rm, dev = 4 * H, ctx.mode, ctx.rowmap, dy1.device
    d_img1 = Bf16Image.empty_rows(H4, rm, mode, dev)
    _persist_bwd(dy1, w_hh1, lens, g1, c1, None, d_img1, mode)
    dy0 = torch.empty(T, B, H, device=dev, dtype=torch.float32)
    gemm_img(d_img1, 0, d_img1.ptr(), w_img, 1, w_img.ptr(), dy0, rm.cap, H, H4, H, rowmap=rm, compact=1)
    dgx0 = torch.empty(T, B, H4, device=dev, dtype=torch.float32) if keep_f32 else None
    d_img0 = Bf16Image.empty_rows(H4, rm, mode, dev)
    _persist_bwd(dy0, w_hh0, lens, g0, c0, dgx0, d_img0, mode)
    return _pair_backward_return(ctx, saved, d_img1, d_img0, dgx0)


def _pair_backward_pipeline(ctx, saved, dy1, w_img, n, keep_f32):
    """DecoderPairFn.backward as a pipeline over n time windows with the sequential form's data flow: BOTH layers' dgates leave their
    recurrences as the whole-sequence batch-major 16-bit images (column sums = the bias gradients; keep_f32: layer 0's as fp32 rows
    beside its image, which the roles kernel writes when it gets both), and chunk c's dX GEMM reads its rows out of layer 1's image
    through a row list (gemm_img a_rows; ChunkGather) -- no fp32 dgates of layer 1, no per-chunk image pass, no second image of the
    whole sequence.  A chunk's list holds rows of that chunk only, all written by the launch in front of the GEMM; the separator rows and
    the zero tail of the images are written by the last launch (the windows with t0 == 0), and only the weight-gradient GEMMs behind it
    read them.
    Carried state: NOT zeroed.  The first window of a layer runs with carry_in = False and never reads it; every non-empty window writes the
    state of every batch row before it ends (also of a group without steps), and the next window of that layer is a later launch on the
    same stream -- what the forward pipeline relies on for its own state."""
    w_hh0, w_ih1, w_hh1, lens, y0, g0, c0, y1, g1, c1 = saved
    T, B, H = y1.shape
    H4, mode, rm = 4 * H, ctx.mode, ctx.rowmap
    dev = dy1.device
    f = dict(device=dev, dtype=torch.float32)
    edges, rms = ctx.chunk_maps
    if n != ctx.nchunks:
        edges = _chunk_edges(T, n)
        rms = _chunk_rowmaps(lens, edges, B)
    assert all(a < b for a, b in zip(edges, edges[1:])), "empty time window in the pair's backward pipeline"
    gr = _chunk_gathers(rms, lens, edges)
    d_img1, d_img0 = Bf16Image.empty_rows(H4, rm, mode, dev), Bf16Image.empty_rows(H4, rm, mode, dev)
    dy0 = torch.empty(T, B, H, **f)
    dgx0 = torch.empty(T, B, H4, **f) if keep_f32 else None
    st = torch.empty(2, B * (H4 + H), **f)                   # per layer: da [B, 4 H] | dc [B, H]
    sb1, sb0 = (st[0, :B * H4], st[0, B * H4:]), (st[1, :B * H4], st[1, B * H4:])
    wb0, wb1 = roles_wimg(w_hh0, mode, True), roles_wimg(w_hh1, mode, True)
    for j in range(n + 1):
        c = n - 1 - j                                        # layer 1's chunk in this launch; layer 0 runs chunk c + 1
        roles = []
        if j < n:
            roles.append(bwd_role(dy1, lens, g1, c1, None, wb1, edges[c], edges[c + 1], sb1, carry_in=c < n - 1, dimg=d_img1))
        if j > 0:
            roles.append(bwd_role(dy0, lens, g0, c0, dgx0, wb0, edges[c + 1], edges[c + 2], sb0, carry_in=c + 1 < n - 1, dimg=d_img0))
        roles_launch(roles, 8 if len(roles) == 2 else 4, mode, dev, backward=True)
        if j < n:
            # dy0 of chunk c = dgates1 W_ih1 over the chunk's valid rows, gathered from the whole-sequence image
            a, b = edges[c], edges[c + 1]
            gemm_img(d_img1, 0, d_img1.ptr(), w_img, 1, w_img.ptr(), dy0[a:b], gr[c].cap, H, H4, H, rowmap=gr[c], compact=1, a_rows=gr[c].a_rows)
    return _pair_backward_return(ctx, saved, d_img1, d_img0, dgx0)


def _input_projection(xs, w_ih, bias, H, reverse, mode, rowmap, fill, gate):
    """A recurrence's input projection gx = [xs] W_ih^T + bias (16-bit rows where gx16_ok allows) as (gx, gates, private).  gates: the
    N = 1 projection of the SAME inputs by gate = (weight [1, K], bias | None), riding on this projection's image where that exists
    (LinearGateFn).  private: gx differentiates through images over this rowmap, so its gradient may come back as the image alone."""
    T, B, N = xs[0].shape[0], xs[0].shape[1], w_ih.shape[0]
    gates = None
    if gx16_ok(mode, rowmap, T, B, H, reverse, xs, N, xs[0].device):
        fill = fill + "|c16"                   # half the bytes the projection writes and the recurrence reads
    if gate is not None and linear_gate_fusable(mode, rowmap, xs, N):
        gx, gates = LinearGateFn.apply(w_ih, bias, gate[0], gate[1], mode, rowmap, fill, *xs)
    else:
        gx = LinearFn.apply(w_ih, bias, L.ACT_NONE, mode, rowmap, fill, *xs)
        if gate is not None:
            gates = linear(xs, gate[0], gate[1], mode=mode)
    private = rowmap is not None and rowmap.T == T and rowmap.B == B and linear_uses_images(mode, T * B, N, xs)
    return gx, gates, private


def decoder_pair(x, lens, p, mode, xs_extra, rowmap, fill, gate, nchunks):
    """the decoder nn.LSTM `p` (two layers) over [x ; xs_extra]: layer 0's input projection (with the gate layer riding on its image,
    lstm_layer) + DecoderPairFn; returns (h, gates)"""
    gx, gates, private = _input_projection([x] + list(xs_extra), p.weight_ih_l0, bias_sum(p.bias_ih_l0, p.bias_hh_l0), p.weight_hh_l0.shape[1],
                                           False, mode, rowmap, fill, gate)
    h = DecoderPairFn.apply(gx, p.weight_hh_l0, p.weight_ih_l1, p.bias_ih_l1, p.bias_hh_l1, p.weight_hh_l1, lens, mode, rowmap, private, nchunks)
    return h, gates


class LSTMSeqFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gx, w_hh, lens, reverse, mode, rowmap=None, gx_private=False):
        """gx_private: gx comes straight from a LinearFn over the same rowmap that differentiates through images (lstm_layer), so
        its gradient may be handed over as the 16-bit image alone"""
        ctx.gx_private = bool(gx_private)
        gx, w_hh = _c(gx), _c(w_hh)
        L.require_cuda(gx, w_hh, lens)
        T, B, H4 = gx.shape
        H = H4 // 4
        ctx.gx_dtype = gx.dtype                       # fp32, or 16-bit rows (lstm_layer: gx16_ok) for the persistent forward kernel
        persistent = lstm_persistent(B, H, reverse, mode, gx.device)
        if gx.dtype != torch.float32 and not persistent:
            gx = gx.float()                           # (the device left the persistent kernels since the projection ran)
        ctx.rowmap = rowmap if (rowmap is not None and not reverse and rowmap.T == T and rowmap.B == B) else None
        y, gates, cell = (torch.empty(T, B, n, device=gx.device, dtype=torch.float32) for n in (H, H4, H))
        if persistent:
            # persistent forward recurrence (csrc/lstm_roles.hip, round 6): rows per XCD group follow the batch -- B <= 32: 4 rows, ONE
            # launch per sequence (1.62 us per step; the round-5 kernel it replaced: 1.76), B <= 64: 8 rows in one launch (1.93 against
            # 2 x 1.76 for two slices), wider: slices of 128 rows at 16 per group (2.77 against 4 x 1.76).  Bit-identical to the
            # launch-per-step kernel for every geometry.
            wimg = roles_wimg(w_hh, mode, False)
            for b0, nb, R in roles_plan(B, False):
                roles_launch([fwd_role(gx, lens, y, gates, cell, wimg, b0=b0, nb=nb)], R, mode, gx.device)
        else:
            work = torch.empty(L.lib().ft_lstm_workspace_bytes(B, H), device=gx.device, dtype=torch.uint8)
            L.check(L.lib().ft_lstm_seq_fwd(L.ptr(gx), L.ptr(w_hh), L.ptr(lens), L.ptr(y), H, L.ptr(gates), L.ptr(cell),
                                            L.ptr(work), T, B, H, int(reverse), mode, L.stream()), "ft_lstm_seq_fwd")
        ctx.save_for_backward(w_hh, lens, y, gates, cell)
        ctx.reverse, ctx.mode = bool(reverse), mode
        return y

    @staticmethod
    def _dgates_roles(ctx, saved, dy):
        """B > 32: slices of 64 rows at 8 per XCD group (2.5 us per step against 2 x 1.65 for two 32-row launches; 16 rows per group lose in
        the backward kernel: 7.2 us per step for 128 rows, profiles/r06_persist_rows_per_group.log)"""
        w_hh, lens, y, gates, cell = saved
        dgx = torch.empty_like(gates)
        wimg = roles_wimg(w_hh, ctx.mode, True)
        for b0, nb, R in roles_plan(y.shape[1], True):
            roles_launch([bwd_role(dy, lens, gates, cell, dgx, wimg, b0=b0, nb=nb)], R, ctx.mode, dy.device, backward=True)
        return dgx, None

    @staticmethod
    def _dgates_reduce_scatter(ctx, saved, dy):
        """B <= 32: the REDUCE-SCATTER kernel (csrc/lstm_persist.hip, round 4: every CU multiplies its own dgates, fp32 partials cross the
        XCD's L2; 1.62 us per step -- the roles backward kernel at 4 rows measures 1.71, so this one stays).  Where the image may leave
        the node (_dgates_exit) and dW_hh runs from compact images, the output waves write the image and its column sums INSTEAD of the
        fp32 rows (beside them where those are kept: 3.07 vs 2.91 us per step): no 450 MB dgx, no conversion pass over it."""
        w_hh, lens, y, gates, cell = saved
        T, B, H = y.shape
        hand, keep_f32 = _dgates_exit(ctx.gx_private)
        emit = hand and ctx.rowmap is not None and ctx.needs_input_grad[1] and T > 1 and images_apply(ctx.mode, 4 * H, H, (T - 1) * B)
        d_img = Bf16Image.empty_rows(4 * H, ctx.rowmap, ctx.mode, dy.device) if emit else None
        dgx = torch.empty_like(gates) if (keep_f32 or not emit) else None
        _persist_bwd(dy, w_hh, lens, gates, cell, dgx, d_img, ctx.mode)
        return dgx, d_img

    @staticmethod
    def _dgates_step(ctx, saved, dy):
        """the launch-per-step kernels (csrc/lstm.hip): either direction, any operand format"""
        w_hh, lens, y, gates, cell = saved
        T, B, H = y.shape
        dgx = torch.empty_like(gates)
        work = torch.empty(L.lib().ft_lstm_workspace_bytes(B, H), device=dy.device, dtype=torch.uint8)
        L.check(L.lib().ft_lstm_seq_bwd(L.ptr(dy), H, L.ptr(w_hh), L.ptr(lens), L.ptr(gates), L.ptr(cell), L.ptr(dgx),
                                        L.ptr(work), T, B, H, int(ctx.reverse), ctx.mode, L.stream()), "ft_lstm_seq_bwd")
        return dgx, None

    @staticmethod
    def backward(ctx, dy):
        saved = w_hh, lens, y, gates, cell = ctx.saved_tensors
        dy = _c(dy)
        T, B, H = y.shape
        persistent = lstm_persistent(B, H, ctx.reverse, ctx.mode, dy.device)
        produce = LSTMSeqFn._dgates_step if not persistent else LSTMSeqFn._dgates_roles if B > 32 else LSTMSeqFn._dgates_reduce_scatter
        dgx, d_img = produce(ctx, saved, dy)           # (fp32 rows | None, compact image | None): no rows = the image is the only form
        # dW_hh[r,j] = sum_{t,b} da_t[b,r] * h_prev(t)[b,j];  h_prev = y[t-1] (fwd) / y[t+1] (reverse)
        dW = weight_grad_out(w_hh) if ctx.needs_input_grad[1] else None
        if dW is not None and (T <= 1 or not images_apply(ctx.mode, 4 * H, H, (T - 1) * B)):
            _dw_other_gradient(w_hh)                    # (zeros, or the fp32-staging GEMM below)
        if dW is not None and T > 1:
            rows, rm, fwd = (T - 1) * B, ctx.rowmap, not ctx.reverse
            if not images_apply(ctx.mode, 4 * H, H, rows):
                gemm_raw(dgx[1:] if fwd else dgx[:-1], y[:-1] if fwd else y[1:], dW, 4 * H, H, rows, 1, 4 * H, H, 1, H, mode=ctx.mode, splitk=True)
            elif rm is not None:
                # compact images (valid frames only, batch-major with one zero separator row per utterance): the one-step shift
                # dgates_t <-> h_{t-1} is a shift by ONE compact row, and the utterance boundaries multiply with a separator
                if d_img is None:
                    d_img = Bf16Image(dgx.reshape(T * B, 4 * H), colsum=True, mode=ctx.mode, rowmap=rm)
                _compact_dw(w_hh, d_img, y_image(y, T * B, H, ctx.mode, rm), dW, 1)
            else:
                # images of dgates / outputs over all T*B rows; the one-step shift is a row offset into them
                d_img, y_img = Bf16Image(dgx.reshape(T * B, 4 * H), colsum=True, mode=ctx.mode), shared_image(y, T * B, H, ctx.mode)
                weight_grad_gemm(w_hh, dW, d_img, d_img.ptr(B if fwd else 0), y_img, y_img.ptr(0 if fwd else B), dW, 4 * H, H, rows, H, beta=1.0)
        return _leave_dgates(dgx, d_img, (T, B, 4 * H), ctx.gx_dtype), dW, None, None, None, None, None


_XPROJ = True     # a narrow input projection (K <= 128) inside the persistent forward recurrence's bursts; tests set it False for the two-kernel path
XPROJ_MAX_K = 128


def xproj_ok(mode, rowmap, T, B, H, reverse, xs, N, gate, device):
    """whether lstm_layer runs projection + recurrence as ONE node whose forward kernel computes gx in its bursts (LSTMProjSeqFn):
    everything gx16_ok asks of the two-kernel path (so the values are the ones that path's 16-bit rows hold), one narrow input, no
    gate layer riding on the projection, and a roles plan of one launch at R <= 8"""
    if not (_XPROJ and gate is None and len(xs) == 1 and xs[0].shape[-1] <= XPROJ_MAX_K and xs[0].shape[-1] % 8 == 0):
        return False
    if not gx16_ok(mode, rowmap, T, B, H, reverse, xs, N, device):
        return False
    plan = roles_plan(B, False)
    return len(plan) == 1 and plan[0][2] <= 8


class _NodeCtx:
    """what a Function's static backward reads of its ctx, for a node that runs the backward of another node as a part of its own"""

    def __init__(self, saved_tensors, needs_input_grad, **attrs):
        self.saved_tensors, self.needs_input_grad = saved_tensors, needs_input_grad
        self.__dict__.update(attrs)


class LSTMProjSeqFn(torch.autograd.Function):
    """y of an LSTM layer from x [T,B,K], K <= 128 (xproj_ok): LinearFn's 16-bit-row projection and LSTMSeqFn's persistent recurrence as one
    node.  The forward makes the operand images LinearFn would make and hands them to the recurrence, whose bursts compute gx (csrc/
    lstm_roles.hip, the XP kernels): no projection GEMM, no [T,B,4H] gx.  y / gates / cell are bit-identical to the two nodes'.  The backward
    IS the two nodes' backward, run one after the other: the same kernels in the same order."""

    @staticmethod
    def forward(ctx, x, w_ih, bias, w_hh, lens, mode, rowmap, fill):
        x, w_ih, bias, w_hh = _c(x), _c(w_ih), _c(bias), _c(w_hh)
        L.require_cuda(x, w_ih, bias, w_hh, lens)
        if bias.data_ptr() % 16:
            bias = bias.clone()                   # (the kernel reads four bias values per lane)
        T, B, K = x.shape
        H = w_hh.shape[1]
        w_img = Bf16Image.of_weight(w_ih, mode)
        x_img = shared_image(x, T * B, K, mode, rowmap)
        y, gates, cell = (torch.empty(T, B, n, device=x.device, dtype=torch.float32) for n in (H, 4 * H, H))
        wimg = roles_wimg(w_hh, mode, False)
        (_, _, R), = roles_plan(B, False)
        roles_launch([fwd_role(None, lens, y, gates, cell, wimg, xproj=(x_img, w_img, bias))], R, mode, x.device)
        ctx.imgs = (w_img, [x_img])
        ctx.save_for_backward(x, w_ih, w_hh, lens, y, gates, cell)
        ctx.mode, ctx.rowmap, ctx.fill = mode, rowmap, fill
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_ih, w_hh, lens, y, gates, cell = ctx.saved_tensors
        need = ctx.needs_input_grad               # x, w_ih, bias, w_hh
        rec = _NodeCtx((w_hh, lens, y, gates, cell), (False, need[3]), reverse=False, mode=ctx.mode, rowmap=ctx.rowmap, gx_private=True,
                       gx_dtype=op16_dtype(ctx.mode))
        dgx, dW_hh = LSTMSeqFn.backward(rec, dy)[:2]
        lin = _NodeCtx((w_ih, None, x), (need[1], need[2], False, False, False, False, need[0]), imgs=ctx.imgs, img_kind="images",
                       lazy_img_mode=None, lazy_src=None, has_bias=True, act=L.ACT_NONE, rowmap=ctx.rowmap, fill=ctx.fill, cat=False,
                       mode=ctx.mode, mode_dx=ctx.mode, mode_dw=ctx.mode)
        g = LinearFn.backward(lin, dgx)
        ctx.imgs = None                           # (a second backward through the graph makes them again: _linear_images_again)
        return g[6], g[0], g[1], dW_hh, None, None, None, None


MAX_STEP_BATCH = 64          # batch rows the launch-per-step recurrences and the bidirectional pair chain take (csrc/lstm.hip)


def batch_chunks(B, cap):
    return [(b0, min(cap, B - b0)) for b0 in range(0, B, cap)]


def lstm_layer(x, lens, w_ih, w_hh, b_ih, b_hh, reverse=False, mode=None, xs_extra=None, rowmap=None, fill="", gate=None):
    """One LSTM layer over a padded sequence: input projection for all T*B rows (valid rows only with a RowMap) as one MFMA
    GEMM, then the sequential recurrence.  The recurrence kernels never use a padded frame's gx / dy row and write zeros to its
    y / dgx row themselves, so the projection leaves padded rows unwritten (fill = ""); pass fill = "dx" when something that
    reduces over all T frames reads the INPUT gradients (the attention context).
    gate = (weight [1, K], bias | None): also returns the N = 1 projection of the SAME inputs (the gate layer, flowtron.py:760-761)
    as (h, gates) -- computed from this projection's operand image where that exists."""
    mode = L.mfma_mode() if mode is None else mode
    xs = [x] if xs_extra is None else [x] + list(xs_extra)
    if reverse:
        rowmap = None
    T, B = x.shape[0], x.shape[1]
    H = w_hh.shape[1]
    if lstm_pad_width(B, H, reverse, mode, x.device, T):
        # a hidden size below the persistent kernels' 1024 (the reference's nn.LSTM takes any, flowtron.py:654-655): the recurrence of a
        # layer whose gate blocks are zero-padded to 1024 units IS this layer's recurrence -- a padded unit has gx = 0 and zero weights,
        # so its cell stays 0 (c = 0.5 c + 0.5 * 0) and its output 0 (0.5 tanh(0)) in every step, and the real units see zeros through
        # zero weight columns.  The padding is torch ops on the parameters: autograd slices the gradients back.
        w_ih_p, w_hh_p, b_p = pad_gate_blocks(w_ih, 0), pad_gate_blocks(w_hh, PERSIST_H - H), pad_gate_blocks(bias_sum(b_ih, b_hh), 0)
        out = lstm_layer(x, lens, w_ih_p, w_hh_p, b_p, torch.zeros_like(b_p), reverse, mode, xs_extra, rowmap, fill, gate)
        return out[..., :H].contiguous() if gate is None else (out[0][..., :H].contiguous(), out[1])
    if xproj_ok(mode, rowmap, T, B, H, reverse, xs, w_ih.shape[0], gate, x.device):
        return LSTMProjSeqFn.apply(x, w_ih, bias_sum(b_ih, b_hh), w_hh, lens, mode, rowmap, fill)
    gx, gates, private = _input_projection(xs, w_ih, bias_sum(b_ih, b_hh), H, reverse, mode, rowmap, fill, gate)
    if B > MAX_STEP_BATCH and not lstm_persistent(B, H, reverse, mode, gx.device):
        # the launch-per-step kernels take at most 64 batch rows (the reference's nn.LSTM takes any, flowtron.py:654-655): the rows
        # are independent, so the recurrence runs per batch chunk on contiguous copies and autograd splits the gradients again
        h = torch.cat([LSTMSeqFn.apply(gx[:, b0:b0 + nb].contiguous(), w_hh, lens[b0:b0 + nb], reverse, mode, None, False)
                       for b0, nb in batch_chunks(B, MAX_STEP_BATCH)], 1)
    else:
        h = LSTMSeqFn.apply(gx, w_hh, lens, reverse, mode, rowmap, private)
    return h if gate is None else (h, gates)


class BiLSTMSeqFn(torch.autograd.Function):
    """[h_fwd | h_rev] of a bidirectional layer, both recurrences in one launch chain (csrc/lstm.hip lstm_*_pair)."""

    @staticmethod
    def forward(ctx, gx_f, gx_r, w_f, w_r, lens, mode=L.FT_BF16):
        ctx.mode = mode
        gx_f, gx_r, w_f, w_r = _c(gx_f), _c(gx_r), _c(w_f), _c(w_r)
        L.require_cuda(gx_f, gx_r, w_f, w_r, lens)
        T, B, H4 = gx_f.shape
        H = H4 // 4
        f = dict(device=gx_f.device, dtype=torch.float32)
        y = torch.empty(T, B, 2 * H, **f)
        gates = [torch.empty(T, B, H4, **f) for _ in range(2)]
        cell = [torch.empty(T, B, H, **f) for _ in range(2)]
        args = (L.ptr(gx_f), L.ptr(gx_r), L.ptr(w_f), L.ptr(w_r), L.ptr(lens), L.ptr(y), 2 * H, L.ptr(gates[0]), L.ptr(gates[1]), L.ptr(cell[0]), L.ptr(cell[1]))
        if bilstm_persist_ok(B, H, mode, gx_f.device):
            st = _persist_watch(gx_f.device)
            work = torch.empty(L.lib().ft_bilstm_persist_workspace_bytes(B, H), device=gx_f.device, dtype=torch.uint8)
            L.check(L.op16("ft_bilstm_persist_fwd", mode)(*args, L.ptr(work), L.ptr(st.status), T, B, H, L.stream()), "ft_bilstm_persist_fwd")
            _persist_arm(st, bilstm=True)
        else:
            nb = L.lib().ft_lstm_workspace_bytes(B, H)
            work = [torch.empty(nb, device=gx_f.device, dtype=torch.uint8) for _ in range(2)]
            L.check(L.op16("ft_lstm_bidir_seq_fwd", mode)(*args, L.ptr(work[0]), L.ptr(work[1]), T, B, H, L.stream()), "ft_lstm_bidir_seq_fwd")
        ctx.save_for_backward(w_f, w_r, lens, y, gates[0], gates[1], cell[0], cell[1])
        return y

    @staticmethod
    def backward(ctx, dy):
        w_f, w_r, lens, y, g0, g1, c0, c1 = ctx.saved_tensors
        dy = _c(dy)
        T, B, H2 = y.shape
        H = H2 // 2
        f = dict(device=dy.device, dtype=torch.float32)
        dgx = [torch.empty(T, B, 4 * H, **f) for _ in range(2)]
        args = (L.ptr(dy), 2 * H, L.ptr(w_f), L.ptr(w_r), L.ptr(lens), L.ptr(g0), L.ptr(g1), L.ptr(c0), L.ptr(c1), L.ptr(dgx[0]), L.ptr(dgx[1]))
        if bilstm_persist_ok(B, H, ctx.mode, dy.device):
            st = _persist_watch(dy.device)
            work = torch.empty(L.lib().ft_bilstm_persist_workspace_bytes(B, H), device=dy.device, dtype=torch.uint8)
            L.check(L.op16("ft_bilstm_persist_bwd", ctx.mode)(*args, L.ptr(work), L.ptr(st.status), T, B, H, L.stream()), "ft_bilstm_persist_bwd")
            _persist_arm(st, bilstm=True)
        else:
            nb = L.lib().ft_lstm_workspace_bytes(B, H)
            work = [torch.empty(nb, device=dy.device, dtype=torch.uint8) for _ in range(2)]
            L.check(L.op16("ft_lstm_bidir_seq_bwd", ctx.mode)(*args, L.ptr(work[0]), L.ptr(work[1]), T, B, H, L.stream()), "ft_lstm_bidir_seq_bwd")
        dWs = [None, None]
        rows = (T - 1) * B
        for d in range(2):
            if ctx.needs_input_grad[2 + d]:
                _dw_other_gradient(w_f if d == 0 else w_r)
                dWs[d] = weight_grad_out(w_f if d == 0 else w_r)         # zero-filled: the GEMM accumulates (beta = 1)
                if T > 1:
                    # dW_hh[r,j] = sum da_t[b,r] h_prev(t)[b,j];  h_prev = y[t-1] (forward) / y[t+1] (reverse), y row stride 2H
                    da = dgx[d][1:] if d == 0 else dgx[d][:-1]
                    hp = y[:-1, :, :H] if d == 0 else y[1:, :, H:]
                    gemm_raw(da, hp, dWs[d], 4 * H, H, rows, 1, 4 * H, 2 * H, 1, H, beta=1.0, mode=ctx.mode, splitk=True)
        return dgx[0], dgx[1], dWs[0], dWs[1], None, None


def bilstm_layer(x, lens, wf, wr, mode=None):
    """Bidirectional LSTM layer.  wf / wr = (w_ih, w_hh, b_ih, b_hh) of the two directions.  Returns [T,B,2H]."""
    mode = L.mfma_mode() if mode is None else mode
    T, B, _ = x.shape
    H = wf[1].shape[1]
    if B > MAX_STEP_BATCH:
        # wider than the recurrence kernels take: batch chunks (independent rows; 32 rows each where the persistent bidirectional
        # kernels apply, else 64), concatenated again -- autograd splits the gradient
        cap = 32 if bilstm_persist_ok(32, H, mode, x.device) else MAX_STEP_BATCH
        return torch.cat([bilstm_layer(x[:, b0:b0 + nb], lens[b0:b0 + nb], wf, wr, mode) for b0, nb in batch_chunks(B, cap)], 1)
    if L.is16(mode) and _os.environ.get("FLOWTRON_BILSTM", "1") != "0" and L.lib().ft_lstm_bidir_supported(B, H):
        gx_f = LinearFn.apply(wf[0], bias_sum(wf[2], wf[3]), L.ACT_NONE, mode, None, "", x)
        gx_r = LinearFn.apply(wr[0], bias_sum(wr[2], wr[3]), L.ACT_NONE, mode, None, "", x)
        return BiLSTMSeqFn.apply(gx_f, gx_r, wf[1], wr[1], lens, mode)
    yf = lstm_layer(x, lens, *wf, reverse=False, mode=mode)
    yb = lstm_layer(x, lens, *wr, reverse=True, mode=mode)
    return torch.cat([yf, yb], 2)


# --------------------------------------------------------------------------
# attention (flowtron.py:544-592)
# --------------------------------------------------------------------------
class AttentionScoresFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Q, K, v, in_lens, prior, temperature):
        Q, K, v = _c(Q), _c(K), _c(v.reshape(-1))
        L.require_cuda(Q, K, v, in_lens, prior)
        T, B, A = Q.shape
        Lk = K.shape[0]
        attn = torch.empty(B, T, Lk, device=Q.device, dtype=torch.float32)
        logprob = torch.empty_like(attn)
        p_save = None
        if prior is not None:
            prior = _c(prior.float())
            p_save = torch.empty_like(attn)
        L.check(L.lib().ft_attention_fwd(L.ptr(Q), L.ptr(K), L.ptr(v), L.ptr(in_lens), L.ptr(prior), L.ptr(attn), L.ptr(logprob),
                                         L.ptr(p_save), T, B, Lk, A, float(temperature), L.stream()), "ft_attention_fwd")
        ctx.save_for_backward(Q, K, v, in_lens, prior, attn, p_save)
        ctx.temperature = float(temperature)
        return attn, logprob

    @staticmethod
    def backward(ctx, dattn, dlogprob):
        Q, K, v, in_lens, prior, attn, p_save = ctx.saved_tensors
        T, B, A = Q.shape
        Lk = K.shape[0]
        if dattn is None:
            dattn = torch.zeros_like(attn)
        dattn = _c(dattn)
        if dlogprob is not None:
            dlogprob = _c(dlogprob)
        de = torch.empty_like(attn)
        dQ = torch.empty_like(Q)
        dK = torch.empty_like(K)
        dv = torch.zeros_like(v)
        L.check(L.lib().ft_attention_bwd(L.ptr(Q), L.ptr(K), L.ptr(v), L.ptr(in_lens), L.ptr(prior), L.ptr(attn), L.ptr(p_save),
                                         L.ptr(dattn), L.ptr(dlogprob), L.ptr(de), L.ptr(dQ), L.ptr(dK), L.ptr(dv),
                                         T, B, Lk, A, ctx.temperature, L.stream()), "ft_attention_bwd")
        return dQ, dK, dv.reshape(1, -1), None, None, None


class ContextFn(torch.autograd.Function):
    """ctx[t,b,:] = sum_l attn[b,t,l] V[l,b,:]  (torch.bmm at flowtron.py:590-591) as one batched MFMA GEMM."""

    @staticmethod
    def forward(ctx, attn, V, mode):
        attn, V = _c(attn), _c(V)
        L.require_cuda(attn, V)
        B, T, Lk = attn.shape
        A = V.shape[2]
        out = torch.empty(T, B, A, device=V.device, dtype=torch.float32)
        gemm_raw(attn, V, out, T, A, Lk, Lk, 1, B * A, 1, B * A, batch=B, bsA=T * Lk, bsB=A, bsC=A, mode=mode)
        ctx.save_for_backward(attn, V)
        ctx.mode = mode
        return out

    @staticmethod
    def backward(ctx, dctx):
        attn, V = ctx.saved_tensors
        dctx = _c(dctx)
        B, T, Lk = attn.shape
        A = V.shape[2]
        dattn = torch.empty_like(attn)
        # dattn[b,t,l] = sum_a dctx[t,b,a] V[l,b,a]
        gemm_raw(dctx, V, dattn, T, Lk, A, B * A, 1, 1, B * A, Lk, batch=B, bsA=A, bsB=A, bsC=T * Lk, mode=ctx.mode)
        dV = torch.empty_like(V)
        # dV[l,b,a] = sum_t attn[b,t,l] dctx[t,b,a]
        gemm_raw(attn, dctx, dV, Lk, A, T, 1, Lk, B * A, 1, B * A, batch=B, bsA=T * Lk, bsB=A, bsC=A, mode=ctx.mode)
        return dattn, dV, None


class CummAttnSeqFn(torch.autograd.Function):
    """run_cumm_attn_sequence (flowtron.py:697-723) as ONE pair of C-ABI calls per flow: the library walks the T dependent frames
    (csrc/cumm_attn.hip: location convolutions, key modulation, per-frame key projection, scores + softmax + context + running
    sum; 8 launches per frame forward, 22 backward, no Python / allocator / autograd work per frame).
    Q [T,B,A] and V [L,B,A] are the projected queries / values, text [L,B,E] the encoder outputs the keys are made from."""

    @staticmethod
    def forward(ctx, Q, V, text, w_key, v, w1, b1, w2, b2, in_lens, temperature, mode):
        Q, V, text, w_key, v, w1, b1, w2, b2 = (_c(t) for t in (Q, V, text, w_key, v.reshape(-1), w1, b1, w2, b2))
        L.require_cuda(Q, V, text, w_key, v, w1, b1, w2, b2, in_lens)
        T, B, A = Q.shape
        Lk, _, E = text.shape
        NF, _, K1 = w1.shape
        K2 = w2.shape[2]
        f = dict(device=Q.device, dtype=torch.float32)
        out_ctx, attn, logprob = torch.empty(T, B, A, **f), torch.empty(B, T, Lk, **f), torch.empty(B, T, Lk, **f)
        cumm_all, kproj_all = torch.empty(T, B, Lk, **f), torch.empty(T, Lk * B, A, **f)
        work = torch.empty(L.lib().ft_cumm_attn_workspace_bytes(T, Lk, B, E, A, NF, K1, K2, int(mode), 0) + 256, device=Q.device, dtype=torch.uint8)
        args = CummAttnSeqFn._args(Q, V, text, w_key, v, w1, b1, w2, b2, in_lens, out_ctx, attn, logprob, cumm_all, kproj_all, work,
                                   temperature, mode)
        # the fused frames as persistent launches (one for all forward frames, one per chunk of backward frames) on a device whose
        # whole-chip grids passed the self-test: same status word, same watch / poison / fallback chain as the persistent recurrences
        st = _persist_watch(Q.device) if (L.is16(mode) and _os.environ.get("FLOWTRON_CUMM_PERSIST", "1") != "0" and persist_usable(Q.device)) else None
        if st is not None:
            args.persist_status = L.ptr(st.status)
        L.check(L.lib().ft_cumm_attn_fwd(C.byref(args), L.stream()), "ft_cumm_attn_fwd")
        if st is not None and L.lib().ft_cumm_attn_fused(C.byref(args)):
            _persist_arm(st)
        ctx.save_for_backward(Q, V, text, w_key, v, w1, b1, w2, b2, in_lens, attn, cumm_all, kproj_all)
        ctx.temperature, ctx.mode = float(temperature), mode
        return out_ctx, attn, logprob

    @staticmethod
    def _args(Q, V, text, w_key, v, w1, b1, w2, b2, in_lens, out_ctx, attn, logprob, cumm_all, kproj_all, work, temperature, mode):
        T, B, A = Q.shape
        Lk, _, E = text.shape
        base = (work.data_ptr() + 255) // 256 * 256
        return L.CummAttnArgs(L.ptr(text), L.ptr(Q), L.ptr(V), L.ptr(w_key), L.ptr(v), L.ptr(w1), L.ptr(b1), L.ptr(w2), L.ptr(b2),
                              L.ptr(in_lens), L.ptr(out_ctx), L.ptr(attn), L.ptr(logprob), L.ptr(cumm_all), L.ptr(kproj_all),
                              base, work.numel() - (base - work.data_ptr()), T, B, Lk, E, A, w1.shape[0], w1.shape[2], w2.shape[2],
                              float(temperature), int(mode), None)

    @staticmethod
    def backward(ctx, dctx, dattn, dlogprob):
        Q, V, text, w_key, v, w1, b1, w2, b2, in_lens, attn, cumm_all, kproj_all = ctx.saved_tensors
        T, B, A = Q.shape
        Lk, _, E = text.shape
        NF, _, K1 = w1.shape
        K2 = w2.shape[2]
        f = dict(device=Q.device, dtype=torch.float32)
        dctx = _c(dctx) if dctx is not None else torch.zeros(T, B, A, **f)
        dattn = _c(dattn) if dattn is not None else None
        dlogprob = _c(dlogprob) if dlogprob is not None else None
        dQ, dV, dtext = torch.empty_like(Q), torch.empty_like(V), torch.empty_like(text)
        dwk, dv, dw1, db1, dw2, db2 = (torch.empty_like(t) for t in (w_key, v, w1, b1, w2, b2))
        work = torch.empty(L.lib().ft_cumm_attn_workspace_bytes(T, Lk, B, E, A, NF, K1, K2, int(ctx.mode), 1) + 256, device=Q.device, dtype=torch.uint8)
        scratch = torch.empty(1, **f)                 # forward-only outputs are not written by the backward call
        args = CummAttnSeqFn._args(Q, V, text, w_key, v, w1, b1, w2, b2, in_lens, scratch, attn, scratch, cumm_all, kproj_all, work,
                                   ctx.temperature, ctx.mode)
        L.check(L.lib().ft_cumm_attn_bwd(C.byref(args), L.ptr(dctx), L.ptr(dattn), L.ptr(dlogprob), L.ptr(dQ), L.ptr(dV), L.ptr(dtext),
                                         L.ptr(dwk), L.ptr(dv), L.ptr(dw1), L.ptr(db1), L.ptr(dw2), L.ptr(db2), L.stream()), "ft_cumm_attn_bwd")
        return dQ, dV, dtext, dwk, dv.reshape(1, -1), dw1, db1, dw2, db2, None, None, None


# --------------------------------------------------------------------------
# affine coupling, reverse-by-length
# --------------------------------------------------------------------------
class AffineFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, out, x):
        out, x = _c(out), _c(x)
        L.require_cuda(out, x)
        M = x.shape[-1]
        rows = x.numel() // M
        z = torch.empty_like(x)
        L.check(L.lib().ft_affine_fwd(L.ptr(out), L.ptr(x), L.ptr(z), rows, M, L.stream()), "ft_affine_fwd")
        ctx.save_for_backward(out, x)
        return z

    @staticmethod
    def backward(ctx, dz):
        out, x = ctx.saved_tensors
        dz = _c(dz)
        M = x.shape[-1]
        rows = x.numel() // M
        dout = torch.empty_like(out)
        dx = torch.empty_like(x)
        L.check(L.lib().ft_affine_bwd(L.ptr(out), L.ptr(x), L.ptr(dz), None, L.ptr(dout), L.ptr(dx), rows, M, L.stream()),
                "ft_affine_bwd")
        return dout, dx


class ReverseByLengthFn(torch.autograd.Function):
    """flip + per-sample roll (flowtron.py:606-613) in closed form; an involution, so backward is the same gather."""

    @staticmethod
    def forward(ctx, x, lens, time_major):
        x = _c(x)
        L.require_cuda(x, lens)
        if time_major:
            T, B, Cc = x.shape
        else:
            B, T, Cc = x.shape
        y = torch.empty_like(x)
        L.check(L.lib().ft_reverse_by_length(L.ptr(x), L.ptr(y), L.ptr(lens), T, B, Cc, int(time_major), L.stream()),
                "ft_reverse_by_length")
        ctx.save_for_backward(lens)
        ctx.time_major = time_major
        return y

    @staticmethod
    def backward(ctx, dy):
        (lens,) = ctx.saved_tensors
        return ReverseByLengthFn.apply(_c(dy), lens, ctx.time_major), None, None


def reverse_by_length(x, lens, time_major=True):
    return ReverseByLengthFn.apply(x, lens, time_major)


# --------------------------------------------------------------------------
# losses (flowtron.py:200-243)
# --------------------------------------------------------------------------
class NLLFn(torch.autograd.Function):
    """[sum m z^2/(2 sigma^2) - sum_f sum m log_s_f] / (n_valid_frames * n_mel).
    log_s tensors are strided views [T,B,M] of the coupling output [T,B,2M] (row stride 2M)."""

    @staticmethod
    def forward(ctx, z, lens, sigma, *log_s):
        z = _c(z)
        L.require_cuda(z, lens)
        T, B, M = z.shape
        acc = torch.zeros(2, device=z.device, dtype=torch.float32)
        st = L.stream()
        L.check(L.lib().ft_masked_sum(L.ptr(z), M, L.ptr(lens), L.ptr(acc), 1, T, B, M, st), "ft_masked_sum")
        lds = []
        for ls in log_s:
            assert ls.shape == z.shape and ls.stride(2) == 1 and ls.stride(1) * B == ls.stride(0)
            lds.append(ls.stride(1))
            L.check(L.lib().ft_masked_sum(L.ptr(ls), ls.stride(1), L.ptr(lens), L.ptr(acc[1:]), 0, T, B, M, st), "ft_masked_sum")
        n = lens_total(lens, float(M))
        nll = (acc[0] / (2.0 * sigma * sigma) - acc[1]) / n
        ctx.save_for_backward(z, lens, n)
        ctx.sigma, ctx.n_ls = sigma, len(log_s)
        return nll

    @staticmethod
    def backward(ctx, g):
        z, lens, n = ctx.saved_tensors
        T, B, M = z.shape
        scale = (g.reshape(1).to(torch.float32) / n).contiguous()
        st = L.stream()
        dz = torch.empty_like(z)
        L.check(L.lib().ft_masked_sum_bwd(L.ptr(z), M, L.ptr(lens), L.ptr(scale), 1.0 / (ctx.sigma * ctx.sigma), 1,
                                          L.ptr(dz), M, T, B, M, st), "ft_masked_sum_bwd")
        dls = None
        if ctx.n_ls:
            dls = torch.empty_like(z)
            L.check(L.lib().ft_masked_sum_bwd(None, M, L.ptr(lens), L.ptr(scale), -1.0, 0, L.ptr(dls), M, T, B, M, st),
                    "ft_masked_sum_bwd")
        return (dz, None, None) + (dls,) * ctx.n_ls


class GateBCEFn(torch.autograd.Function):
    """sum_valid BCEWithLogits(gate, target) / n_valid_frames (flowtron.py:237-243). gate [T,B,1], target [B,T]."""

    @staticmethod
    def forward(ctx, gate, target, lens):
        gate, target = _c(gate), _c(target.float())
        L.require_cuda(gate, target, lens)
        T, B = gate.shape[0], gate.shape[1]
        acc = torch.zeros(1, device=gate.device, dtype=torch.float32)
        L.check(L.lib().ft_gate_bce_fwd(L.ptr(gate), L.ptr(target), L.ptr(lens), L.ptr(acc), T, B, L.stream()), "ft_gate_bce_fwd")
        n = lens_total(lens)
        ctx.save_for_backward(gate, target, lens, n)
        return (acc / n).reshape(())

    @staticmethod
    def backward(ctx, g):
        gate, target, lens, n = ctx.saved_tensors
        T, B = gate.shape[0], gate.shape[1]
        scale = (g.reshape(1).to(torch.float32) / n).contiguous()
        dgate = torch.empty_like(gate)
        L.check(L.lib().ft_gate_bce_bwd(L.ptr(gate), L.ptr(target), L.ptr(lens), L.ptr(scale), 1.0, L.ptr(dgate), T, B, L.stream()),
                "ft_gate_bce_bwd")
        return dgate, None, None


# --------------------------------------------------------------------------
# beta-binomial attention prior on device (data.py:31-41; the reference spends ~0.45 s/utterance in scipy)
# --------------------------------------------------------------------------
def beta_binomial_prior(in_lens, out_lens, T=None, Lk=None, scaling=1.0):
    """-> [B,T,L] fp32 prior for a whole batch, zero padded like DataCollate (data.py:225-243)."""
    L.require_cuda(in_lens, out_lens)
    i32, o32 = lens32(in_lens), lens32(out_lens)
    B = i32.numel()
    if T is None:
        T = int(out_lens.max())
    if Lk is None:
        Lk = int(in_lens.max())
    prior = torch.empty(B, T, Lk, device=i32.device, dtype=torch.float32)
    L.check(L.lib().ft_beta_binomial_prior(L.ptr(i32), L.ptr(o32), L.ptr(prior), B, T, Lk, float(scaling), L.stream()),
            "ft_beta_binomial_prior")
    return prior


# --------------------------------------------------------------------------
# elementwise add / mul (cumulative-attention branch, flowtron.py:712, :719)
# --------------------------------------------------------------------------
def _elt(a, b, op):
    out = torch.empty_like(a)
    L.check(L.lib().ft_eltwise(L.ptr(a), L.ptr(b), L.ptr(out), a.numel(), op, L.stream()), "ft_eltwise")
    return out


class MulFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        L.require_cuda(a, b)
        assert a.shape == b.shape
        ctx.save_for_backward(a, b)
        return _elt(a, b, 1)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = _c(g)
        return (_elt(g, b, 1) if ctx.needs_input_grad[0] else None), (_elt(g, a, 1) if ctx.needs_input_grad[1] else None)


class AddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a, b = _c(a), _c(b)
        L.require_cuda(a, b)
        assert a.shape == b.shape
        return _elt(a, b, 0)

    @staticmethod
    def backward(ctx, g):
        return g, g


# --------------------------------------------------------------------------
# attention-CTC loss (flowtron.py:155-182): banded DP kernel, one workgroup per sample
# --------------------------------------------------------------------------
class AttnCTCFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, lp, in_lens32, out_lens32, blank_logprob):
        lp = _c(lp.float())
        L.require_cuda(lp, in_lens32, out_lens32)
        B, T, Lk = lp.shape
        work = torch.empty(L.lib().ft_attn_ctc_workspace_floats(B, T, Lk), device=lp.device, dtype=torch.float32)
        loss = torch.empty(1, device=lp.device, dtype=torch.float32)
        ctx.with_beta = int(bool(ctx.needs_input_grad[0]))       # beta recursion beside alpha, in the same launch
        L.check(L.lib().ft_attn_ctc_fwd(L.ptr(lp), L.ptr(in_lens32), L.ptr(out_lens32), float(blank_logprob), L.ptr(work),
                                        L.ptr(loss), B, T, Lk, ctx.with_beta, L.stream()), "ft_attn_ctc_fwd")
        ctx.save_for_backward(lp, in_lens32, out_lens32, work)
        ctx.blank = float(blank_logprob)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        lp, in32, out32, work = ctx.saved_tensors
        B, T, Lk = lp.shape
        gd = g.reshape(1).to(torch.float32).contiguous()
        dlp = torch.empty_like(lp)
        L.check(L.lib().ft_attn_ctc_bwd(L.ptr(lp), L.ptr(in32), L.ptr(out32), ctx.blank, L.ptr(work), L.ptr(gd), L.ptr(dlp),
                                        B, T, Lk, ctx.with_beta, L.stream()), "ft_attn_ctc_bwd")
        return dlp, None, None, None


# --------------------------------------------------------------------------
# FlowtronLoss as ONE autograd node (flowtron.py:200-274): NLL + gate + attention-CTC of all flows
# --------------------------------------------------------------------------
FUSED_LOSS = True


def _ptr_array(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class FlowtronLossFn(torch.autograd.Function):
    """(nll, gate_loss, ctc) from seven launches, their gradients from three -- where NLLFn + GateBCEFn + AttnCTCFn and the torch
    arithmetic around them (frame counts, normalisers, `g / n`, the concatenation of the flows' log-probabilities, the flip of the
    back-step flows', `lens.repeat(F)`) took ~55 dispatches of 4-20 us per training step, most of them in front of the host's
    .item() reads (train.py:300-303) and at the head of backward, where the GPU waits for the host.
    tensors = n_ls log_s views [T,B,M] (strided views of the coupling outputs) followed by the flows' attention log-probabilities
    [B,T,L] in flows order, each in ITS flow's time order (odd flows reversed: ft_attn_ctc_fwd_multi mirrors the row index)."""

    @staticmethod
    def forward(ctx, z, gate_pred, gate_target, out32, in32, sigma, blank, n_ls, *tensors):
        z = _c(z)
        log_s, lps = list(tensors[:n_ls]), [_c(t) for t in tensors[n_ls:]]
        L.require_cuda(z, gate_pred, gate_target, out32, in32, *log_s, *lps)
        T, B, M = z.shape
        dev = z.device
        st = L.stream()
        ld = M
        for ls in log_s:
            assert ls.shape == z.shape and ls.dtype == torch.float32 and ls.stride(2) == 1 and ls.stride(1) * B == ls.stride(0)
        if log_s:
            ld = int(log_s[0].stride(1))
            assert all(int(ls.stride(1)) == ld for ls in log_s)
        acc = torch.empty(8, device=dev, dtype=torch.float32)
        nll = torch.empty((), device=dev, dtype=torch.float32)
        gate_loss = None
        if gate_pred is not None:
            gate_pred, gate_target = _c(gate_pred), _c(gate_target.float())
            assert gate_pred.numel() == T * B and gate_target.shape == (B, T)
            gate_loss = torch.empty((), device=dev, dtype=torch.float32)
        L.check(L.lib().ft_flowtron_loss_fwd(L.ptr(z), _ptr_array(log_s) if log_s else None, len(log_s), ld, L.ptr(gate_pred),
                                             L.ptr(gate_target), L.ptr(out32), float(sigma), L.ptr(acc), L.ptr(nll), L.ptr(gate_loss),
                                             T, B, M, st), "ft_flowtron_loss_fwd")
        ctc = work = None
        ctx.with_beta = 0
        if lps:
            F_, (Bl, Tl, Lk) = len(lps), lps[0].shape
            assert Bl == B and all(lp.shape == lps[0].shape and lp.dtype == torch.float32 for lp in lps)
            ctx.rev = (C.c_int32 * F_)(*[f % 2 for f in range(F_)])          # back-step flows: reversed time (flowtron.py:250-256)
            ctx.with_beta = int(any(ctx.needs_input_grad[8 + n_ls + f] for f in range(F_)))
            work = torch.empty(L.lib().ft_attn_ctc_workspace_floats(F_ * B, Tl, Lk), device=dev, dtype=torch.float32)
            ctc = torch.empty((), device=dev, dtype=torch.float32)
            L.check(L.lib().ft_attn_ctc_fwd_multi(_ptr_array(lps), ctx.rev, F_, L.ptr(in32), L.ptr(out32), float(blank), L.ptr(work),
                                                  L.ptr(ctc), B, Tl, Lk, ctx.with_beta, st), "ft_attn_ctc_fwd_multi")
        ctx.save_for_backward(z, gate_pred, gate_target, out32, in32, acc, work, *lps)
        ctx.sigma, ctx.blank, ctx.n_ls, ctx.n_lp = float(sigma), float(blank), n_ls, len(lps)
        outs = (nll, gate_loss if gate_loss is not None else torch.zeros(1, device=dev),
                ctc if ctc is not None else torch.zeros(1, device=dev))
        ctx.mark_non_differentiable(*[o for o, live in zip(outs[1:], (gate_loss is not None, ctc is not None)) if not live])
        return outs

    @staticmethod
    def backward(ctx, g_nll, g_gate, g_ctc):
        z, gate_pred, gate_target, out32, in32, acc, work, *lps = ctx.saved_tensors
        T, B, M = z.shape
        st = L.stream()

        def scalar(g):
            return None if g is None else _c(g.reshape(1).to(torch.float32))

        g_nll = scalar(g_nll) if (ctx.needs_input_grad[0] or any(ctx.needs_input_grad[8:8 + ctx.n_ls])) else None
        g_gate = scalar(g_gate) if (gate_pred is not None and ctx.needs_input_grad[1]) else None
        dz = dls = dgate = None
        if g_nll is not None:
            dz = torch.empty_like(z)
            dls = torch.empty_like(z) if ctx.n_ls else None
        if g_gate is not None:
            dgate = torch.empty_like(gate_pred)
        if dz is not None or dgate is not None:
            L.check(L.lib().ft_flowtron_loss_bwd(L.ptr(z), L.ptr(gate_pred), L.ptr(gate_target), L.ptr(out32), ctx.sigma, L.ptr(acc),
                                                 L.ptr(g_nll), L.ptr(g_gate), L.ptr(dz), L.ptr(dls), L.ptr(dgate), T, B, M, st),
                    "ft_flowtron_loss_bwd")
        dlps = [None] * ctx.n_lp
        if lps and g_ctc is not None and any(ctx.needs_input_grad[8 + ctx.n_ls:]):
            g_ctc = scalar(g_ctc)
            dlps = [torch.empty_like(lp) for lp in lps]
            _, Tl, Lk = lps[0].shape
            L.check(L.lib().ft_attn_ctc_bwd_multi(_ptr_array(lps), ctx.rev, len(lps), L.ptr(in32), L.ptr(out32), ctx.blank, L.ptr(work),
                                                  L.ptr(g_ctc), _ptr_array(dlps), B, Tl, Lk, ctx.with_beta, st), "ft_attn_ctc_bwd_multi")
        return (dz, dgate, None, None, None, None, None, None) + (dls,) * ctx.n_ls + tuple(dlps)


# --------------------------------------------------------------------------
# two stacked LSTM layers as one launch chain (csrc/lstm2.hip)
# --------------------------------------------------------------------------
class LSTM2SeqFn(torch.autograd.Function):
    """y1 = LSTM_l1(LSTM_l0(gx0)); gx0 = x W_ih0^T + b0 comes from LinearFn.  bf16 MFMA operands, forward direction."""

    @staticmethod
    def forward(ctx, gx0, w_hh0, w_ih1, b_ih1, b_hh1, w_hh1, lens, mode=L.FT_BF16):
        ctx.mode = mode
        gx0, w_hh0, w_ih1, w_hh1 = _c(gx0), _c(w_hh0), _c(w_ih1), _c(w_hh1)
        L.require_cuda(gx0, w_hh0, w_ih1, w_hh1, lens)
        T, B, H4 = gx0.shape
        H = H4 // 4
        f = dict(device=gx0.device, dtype=torch.float32)
        y0, y1 = torch.empty(T, B, H, **f), torch.empty(T, B, H, **f)
        gates0, gates1 = torch.empty(T, B, H4, **f), torch.empty(T, B, H4, **f)
        cell0, cell1 = torch.empty(T, B, H, **f), torch.empty(T, B, H, **f)
        bias1 = (b_ih1 + b_hh1).contiguous()
        work = torch.empty(L.lib().ft_lstm2_workspace_bytes(B, H), device=gx0.device, dtype=torch.uint8)
        L.check(L.op16("ft_lstm2_seq_fwd", mode)(L.ptr(gx0), L.ptr(w_hh0), L.ptr(w_ih1), L.ptr(bias1), L.ptr(w_hh1), L.ptr(lens), L.ptr(y0),
                                         L.ptr(gates0), L.ptr(cell0), L.ptr(y1), L.ptr(gates1), L.ptr(cell1), L.ptr(work), T, B, H,
                                         L.stream()), "ft_lstm2_seq_fwd")
        ctx.save_for_backward(w_hh0, w_ih1, w_hh1, lens, y0, gates0, cell0, y1, gates1, cell1)
        return y1

    @staticmethod
    def backward(ctx, dy1):
        w_hh0, w_ih1, w_hh1, lens, y0, gates0, cell0, y1, gates1, cell1 = ctx.saved_tensors
        dy1 = _c(dy1)
        T, B, H = y1.shape
        dgx0 = torch.empty(T, B, 4 * H, device=dy1.device, dtype=torch.float32)
        dgx1 = torch.empty_like(dgx0)
        work = torch.empty(L.lib().ft_lstm2_workspace_bytes(B, H), device=dy1.device, dtype=torch.uint8)
        L.check(L.op16("ft_lstm2_seq_bwd", ctx.mode)(L.ptr(dy1), L.ptr(w_hh0), L.ptr(w_ih1), L.ptr(w_hh1), L.ptr(lens), L.ptr(gates0), L.ptr(cell0),
                                         L.ptr(gates1), L.ptr(cell1), L.ptr(dgx0), L.ptr(dgx1), L.ptr(work), T, B, H, L.stream()),
                "ft_lstm2_seq_bwd")
        mode = ctx.mode
        rows = T * B
        dW_hh0 = torch.zeros_like(w_hh0)
        dW_hh1 = torch.zeros_like(w_hh1)
        dW_ih1 = torch.empty_like(w_ih1)
        r1 = (T - 1) * B
        db1 = None
        if T > 1 and images_apply(mode, 4 * H, H, r1):
            # four images serve the three weight-gradient GEMMs (the one-step shift is a row offset) and, through the
            # hand-off, the dX / dW GEMMs of the layer-0 input projection
            d0, d1 = Bf16Image(dgx0.reshape(rows, 4 * H), colsum=True, mode=mode), Bf16Image(dgx1.reshape(rows, 4 * H), colsum=True, mode=mode)
            i0, i1 = Bf16Image(y0.reshape(rows, H), mode=mode), shared_image(y1, rows, H, mode)
            weight_grad_gemm(w_hh0, dW_hh0, d0, d0.ptr(B), i0, i0.ptr(), dW_hh0, 4 * H, H, r1, H)
            weight_grad_gemm(w_hh1, dW_hh1, d1, d1.ptr(B), i1, i1.ptr(), dW_hh1, 4 * H, H, r1, H)
            weight_grad_gemm(w_ih1, dW_ih1, d1, d1.ptr(), i0, i0.ptr(), dW_ih1, 4 * H, H, rows, H)
            _handoff_put(dgx0, d0)
            db1 = d1.colsum
        else:
            for w in (w_hh0, w_hh1, w_ih1):
                _dw_other_gradient(w)
            if T > 1:
                gemm_raw(dgx0[1:], y0[:-1], dW_hh0, 4 * H, H, r1, 1, 4 * H, H, 1, H, mode=mode, splitk=True)
                gemm_raw(dgx1[1:], y1[:-1], dW_hh1, 4 * H, H, r1, 1, 4 * H, H, 1, H, mode=mode, splitk=True)
            gemm_raw(dgx1, y0, dW_ih1, 4 * H, H, rows, 1, 4 * H, H, 1, H, mode=mode, splitk=True)
        if db1 is None:
            db1 = colsum(dgx1, rows, 4 * H, 4 * H)
        return dgx0, dW_hh0, dW_ih1, db1, db1, dW_hh1, None, None


def lstm2_supported(B, H, mode):
    return L.is16(mode) and _os.environ.get("FLOWTRON_LSTM2", "1") != "0" and bool(L.lib().ft_lstm2_supported(B, H))


# --------------------------------------------------------------------------
# style transfer: posterior over z from reference utterances (inference_style_transfer.ipynb; csrc/style.hip)
# --------------------------------------------------------------------------
def style_accumulate(z, lens32_, acc, n_frames, mode):
    """acc (float64, [M, n_frames] or [M]) += the B utterances of z [B,M,T] fp32 of ANY strides (read in place), in order of b."""
    L.require_cuda(z, lens32_, acc)
    B, M, T = z.shape
    sb, sm, st = z.stride()
    L.check(L.lib().ft_style_accumulate(L.ptr(z), sb, sm, st, L.ptr(lens32_), L.ptr(acc), B, M, T, n_frames, mode, L.stream()),
            "ft_style_accumulate")


def style_sample(acc, count, lambd, M, n_frames, mode, eps=None, sigma=0.0):
    """-> fp32 [S, M, n_frames] = mu + sigma * eps (eps [S,M,n_frames] fp32 contiguous), or mu itself [1, M, n_frames] without eps."""
    L.require_cuda(acc, eps)
    S = 1 if eps is None else eps.shape[0]
    out = torch.empty(S, M, n_frames, device=acc.device, dtype=torch.float32)
    L.check(L.lib().ft_style_sample(L.ptr(acc), L.ptr(eps), L.ptr(out), S, M, n_frames, count, float(lambd), float(sigma), mode,
                                    L.stream()), "ft_style_sample")
    return out


# --------------------------------------------------------------------------
# token durations and alignments from durations (csrc/align.hip)
# --------------------------------------------------------------------------
def mas_ragged(logp, in32, out32, want_score=False):
    """Monotonic alignment search of a ragged batch: logp [B,T,L] fp32 of ANY strides (read in place), device int32 lengths ->
    (path [B,T] int32, durations [B,L] int32, score [B] fp32 | None)."""
    L.require_cuda(logp, in32, out32)
    B, T, Lt = logp.shape
    dev = logp.device
    path = torch.empty(B, T, device=dev, dtype=torch.int32)
    dur = torch.empty(B, Lt, device=dev, dtype=torch.int32)
    score = torch.empty(B, device=dev, dtype=torch.float32) if want_score else None
    nbytes = L.lib().ft_mas_workspace_bytes(B, T, Lt)
    work = torch.empty(nbytes // 8, device=dev, dtype=torch.int64)
    sb, st, sl = logp.stride()
    L.check(L.lib().ft_mas_ragged(L.ptr(logp), sb, st, sl, L.ptr(in32), L.ptr(out32), L.ptr(path), L.ptr(dur), L.ptr(score),
                                  L.ptr(work), nbytes, B, T, Lt, L.stream()), "ft_mas_ragged")
    return path, dur, score


def durations_to_rows(dur32, in32, n_frames, reverse=False):
    """durations [B,L] int32 contiguous -> one-hot alignment rows [B, n_frames, L] fp32 (reverse: each utterance's own frames in
    reversed time), zeros behind an utterance's total and its tokens."""
    L.require_cuda(dur32, in32)
    B, Lt = dur32.shape
    rows = torch.empty(B, n_frames, Lt, device=dur32.device, dtype=torch.float32)
    L.check(L.lib().ft_durations_to_rows(L.ptr(dur32), L.ptr(in32), L.ptr(rows), B, n_frames, Lt, int(bool(reverse)), L.stream()),
            "ft_durations_to_rows")
    return rows


# --------------------------------------------------------------------------
# attention diagnostics (csrc/score.hip; the frame log-likelihood beside it is bound in flowtron_amd/score.py)
# --------------------------------------------------------------------------
def attn_diagnostics(attn, in32, out32):
    """attn [F,B,T,L] fp32 of ANY strides (read in place, natural time), device int32 lengths -> (peaks [F,B,T] int32, -1 behind
    out_lens; counters [F,B,6] int32: n_attended, n_backward, n_skipped, longest_run, first_peak, last_peak; focus_sum [F,B]
    float64)."""
    L.require_cuda(attn, in32, out32)
    F_, B, T, Lt = attn.shape
    dev = attn.device
    peaks = torch.empty(F_, B, T, device=dev, dtype=torch.int32)
    counters = torch.empty(F_, B, 6, device=dev, dtype=torch.int32)
    focus = torch.empty(F_, B, device=dev, dtype=torch.float64)
    nbytes = L.lib().ft_attn_diagnostics_workspace_bytes(F_, B, Lt)
    work = torch.empty(nbytes // 4, device=dev, dtype=torch.int32)
    sf, sb, st, sl = attn.stride()
    L.check(L.lib().ft_attn_diagnostics(L.ptr(attn), sf, sb, st, sl, L.ptr(in32), L.ptr(out32), L.ptr(peaks), L.ptr(counters),
                                        L.ptr(focus), L.ptr(work), nbytes, F_, B, T, Lt, L.stream()), "ft_attn_diagnostics")
    return peaks, counters, focus


# --------------------------------------------------------------------------
# mel-cepstral distortion along a dynamic-time-warping path (csrc/dtw.hip)
# --------------------------------------------------------------------------
def mel_cepstra(mel, lens32_, dct):
    """mel [B,M,T] fp32 of ANY strides (read in place), device int32 frame counts or None, dct [K,M] fp32 contiguous ->
    cepstra [B,T,K] fp32; rows at or behind lens stay 0."""
    L.require_cuda(mel, lens32_, dct)
    B, M, T = mel.shape
    K = dct.shape[0]
    cep = torch.zeros(B, T, K, device=mel.device, dtype=torch.float32)
    sb, sm, st = mel.stride()
    L.check(L.lib().ft_mel_cepstra(L.ptr(mel), sb, sm, st, L.ptr(lens32_), L.ptr(dct), L.ptr(cep), B, M, T, K, L.stream()),
            "ft_mel_cepstra")
    return cep


def dtw_ragged(x, y, x32, y32, diagonal=False):
    """Dynamic time warping of a ragged batch of pairs: x [B,Ta,K], y [B,Tb,K] fp32 of ANY strides (read in place), device int32
    lengths -> (cost [B] fp32, path [B, Ta+Tb-1, 2] int32 with -1 behind path_len, path_len [B] int32)."""
    L.require_cuda(x, y, x32, y32)
    B, Ta, K = x.shape
    Tb = y.shape[1]
    dev = x.device
    cost = torch.empty(B, device=dev, dtype=torch.float32)
    path_len = torch.empty(B, device=dev, dtype=torch.int32)
    path = torch.empty(B, Ta + Tb - 1, 2, device=dev, dtype=torch.int32)
    nbytes = L.lib().ft_dtw_workspace_bytes(B, Ta, Tb, K)
    work = torch.empty(max(nbytes // 8, 2), device=dev, dtype=torch.int64)
    L.check(L.lib().ft_dtw_ragged(L.ptr(x), *x.stride(), L.ptr(y), *y.stride(), L.ptr(x32), L.ptr(y32), L.ptr(cost),
                                  L.ptr(path_len), L.ptr(path), L.ptr(work), nbytes, B, Ta, Tb, K, int(bool(diagonal)), L.stream()),
            "ft_dtw_ragged")
    return cost, path, path_len


# --------------------------------------------------------------------------
# F0 tracking (YIN) and F0 error along a warping path (csrc/pitch.hip)
# --------------------------------------------------------------------------
def f0_yin_ragged(audio, n32, sampling_rate, hop, W, tau_min, tau_max, threshold):
    """audio [B,N] fp32 of ANY strides (read in place), device int32 sample counts -> (f0 [B,T] fp32 Hz, 0 = unvoiced,
    aperiodicity [B,T] fp32), T = N // hop + 1, zeros behind an utterance's n // hop + 1 frames."""
    L.require_cuda(audio, n32)
    B, N = audio.shape
    T = N // hop + 1
    f0 = torch.empty(B, T, device=audio.device, dtype=torch.float32)
    ap = torch.empty(B, T, device=audio.device, dtype=torch.float32)
    L.check(L.lib().ft_f0_yin_ragged(L.ptr(audio), *audio.stride(), L.ptr(n32), L.ptr(f0), L.ptr(ap), B, N, float(sampling_rate),
                                     hop, W, tau_min, tau_max, float(threshold), L.stream()), "ft_f0_yin_ragged")
    return f0, ap


def f0_candidates_ragged(audio, n32, cum, lag_edges, sampling_rate, hop, W, tau_min, tau_max, absolute_min_prob):
    """audio [B,N] fp32 of ANY strides, device int32 sample counts, cum [101] and lag_edges [n_bins + 1] fp32 on the device ->
    (prob [B,T,n_bins], freq [B,T,n_bins] Hz, voiced_prob [B,T]) fp32, zeros behind an utterance's frames.  One launch."""
    L.require_cuda(audio, n32, cum, lag_edges)
    B, N = audio.shape
    T, n_bins = N // hop + 1, lag_edges.numel() - 1
    prob = torch.empty(B, T, n_bins, device=audio.device, dtype=torch.float32)
    freq = torch.empty(B, T, n_bins, device=audio.device, dtype=torch.float32)
    voiced = torch.empty(B, T, device=audio.device, dtype=torch.float32)
    L.check(L.lib().ft_f0_candidates_ragged(L.ptr(audio), *audio.stride(), L.ptr(n32), L.ptr(cum), L.ptr(lag_edges), L.ptr(prob),
                                            L.ptr(freq), L.ptr(voiced), B, N, float(sampling_rate), hop, W, tau_min, tau_max, n_bins,
                                            float(absolute_min_prob), L.stream()), "ft_f0_candidates_ragged")
    return prob, freq, voiced


def f0_viterbi_ragged(prob, freq, voiced, n32, transition, centres, N, hop, switch_prob):
    """what f0_candidates_ragged wrote (contiguous), transition [2 band + 1] and centres [n_bins] fp32 on the device ->
    f0 [B,T] fp32 Hz, 0 = unvoiced and behind an utterance's frames.  One launch."""
    L.require_cuda(prob, freq, voiced, n32, transition, centres)
    B, T, n_bins = prob.shape
    f0 = torch.empty(B, T, device=prob.device, dtype=torch.float32)
    nbytes = L.lib().ft_f0_viterbi_workspace_bytes(B, T, n_bins)
    work = torch.empty(nbytes, device=prob.device, dtype=torch.uint8)
    L.check(L.lib().ft_f0_viterbi_ragged(L.ptr(prob), L.ptr(freq), L.ptr(voiced), L.ptr(n32), L.ptr(transition), L.ptr(centres),
                                         L.ptr(f0), L.ptr(work), nbytes, B, N, hop, n_bins, (transition.numel() - 1) // 2,
                                         float(switch_prob), L.stream()), "ft_f0_viterbi_ragged")
    return f0


def f0_path_stats(f0_a, f0_b, path, path_len):
    """f0_a [B,Ta], f0_b [B,Tb] fp32 of ANY strides, path [B,P,2] int32 contiguous, path_len [B] int32 -> (n_both [B] int32,
    n_mismatch [B] int32, sum_sq [B] float64: squared cents over the cells where both frames are voiced)."""
    L.require_cuda(f0_a, f0_b, path, path_len)
    B, Ta = f0_a.shape
    Tb, P = f0_b.shape[1], path.shape[1]
    dev = f0_a.device
    n_both = torch.empty(B, device=dev, dtype=torch.int32)
    n_mismatch = torch.empty(B, device=dev, dtype=torch.int32)
    sum_sq = torch.empty(B, device=dev, dtype=torch.float64)
    L.check(L.lib().ft_f0_path_stats(L.ptr(f0_a), *f0_a.stride(), L.ptr(f0_b), *f0_b.stride(), L.ptr(path), L.ptr(path_len),
                                     L.ptr(n_both), L.ptr(n_mismatch), L.ptr(sum_sq), B, Ta, Tb, P, L.stream()), "ft_f0_path_stats")
    return n_both, n_mismatch, sum_sq


# --------------------------------------------------------------------------
# Gaussian-mixture prior (flowtron.py:217-231, 312-363, 437-439; csrc/mixture.hip)
# --------------------------------------------------------------------------
class TimePoolFn(torch.autograd.Function):
    """y[b] = sum_{t < lens[b]} x[t, b] / max(lens): the reference's torch.mean over the time axis of the zero-padded BiLSTM
    output (flowtron.py:437-439) -- the divisor is the batch's LONGEST length, taken on the device.  x [T,B,W] -> [B,W]."""

    @staticmethod
    def forward(ctx, x, lens):
        x = _c(x)
        L.require_cuda(x, lens)
        T, B, W = x.shape
        y = torch.empty(B, W, device=x.device, dtype=torch.float32)
        L.check(L.lib().ft_time_pool_fwd(L.ptr(x), L.ptr(lens), L.ptr(y), T, B, W, L.stream()), "ft_time_pool_fwd")
        ctx.save_for_backward(lens)
        ctx.T = T
        return y

    @staticmethod
    def backward(ctx, dy):
        lens, = ctx.saved_tensors
        dy = _c(dy)
        B, W = dy.shape
        dx = torch.empty(ctx.T, B, W, device=dy.device, dtype=torch.float32)
        L.check(L.lib().ft_time_pool_bwd(L.ptr(dy), L.ptr(lens), L.ptr(dx), ctx.T, B, W, L.stream()), "ft_time_pool_bwd")
        return dx, None


class SoftmaxRowsFn(torch.autograd.Function):
    """softmax over the components of each row: [B,C] -> [B,C], 2 <= C <= 64 (flowtron.py:352)."""

    @staticmethod
    def forward(ctx, x):
        x = _c(x)
        L.require_cuda(x)
        B, Cn = x.shape
        y = torch.empty_like(x)
        L.check(L.lib().ft_softmax_rows_fwd(L.ptr(x), L.ptr(y), B, Cn, L.stream()), "ft_softmax_rows_fwd")
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, = ctx.saved_tensors
        dy = _c(dy)
        B, Cn = y.shape
        dx = torch.empty_like(y)
        L.check(L.lib().ft_softmax_rows_bwd(L.ptr(y), L.ptr(dy), L.ptr(dx), B, Cn, L.stream()), "ft_softmax_rows_bwd")
        return dx


class MixtureNLLFn(torch.autograd.Function):
    """[-sum m log sum_c prob_c N(z; mean_c, exp(log_var_c)) - sum_f sum m log_s_f] / (n_valid_frames * n_mel), the Gaussians
    without their 2 pi term (flowtron.py:217-235).  z [T,B,M]; mean, log_var [1,M,C] (fixed) or [B,M,C]; prob [B,C]; log_s: strided
    views [T,B,M] of the coupling outputs.  One node: gradients to z, every log_s and -- where asked for -- mean, log_var, prob."""

    @staticmethod
    def forward(ctx, z, mean, log_var, prob, lens, *log_s):
        z, mean, log_var, prob = _c(z), _c(mean), _c(log_var), _c(prob)
        L.require_cuda(z, mean, log_var, prob, lens, *log_s)
        T, B, M = z.shape
        Bm, Cn = mean.shape[0], mean.shape[2]
        if tuple(mean.shape) != (Bm, M, Cn) or log_var.shape != mean.shape or tuple(prob.shape) != (B, Cn):
            raise ValueError("mixture shapes: mean / log_var [1 or B, M, C] and prob [B, C] for z [T, B, M], got %s, %s, %s, %s"
                             % (tuple(mean.shape), tuple(log_var.shape), tuple(prob.shape), tuple(z.shape)))
        ld = M
        for ls in log_s:
            assert ls.shape == z.shape and ls.dtype == torch.float32 and ls.stride(2) == 1 and ls.stride(1) * B == ls.stride(0)
        if log_s:
            ld = int(log_s[0].stride(1))
            assert all(int(ls.stride(1)) == ld for ls in log_s)
        dev = z.device
        acc = torch.empty(8, device=dev, dtype=torch.float32)
        loss = torch.empty((), device=dev, dtype=torch.float32)
        nw = L.lib().ft_mixture_nll_work_floats(T, B, M, Cn)
        work = torch.empty(max(nw, 1), device=dev, dtype=torch.float32)
        L.check(L.lib().ft_mixture_nll_fwd(L.ptr(z), L.ptr(mean), L.ptr(log_var), L.ptr(prob), _ptr_array(log_s) if log_s else None,
                                           len(log_s), ld, L.ptr(lens), L.ptr(acc), L.ptr(work), L.ptr(loss), T, B, M, Cn, Bm,
                                           L.stream()), "ft_mixture_nll_fwd")
        ctx.save_for_backward(z, mean, log_var, prob, lens, acc)
        ctx.n_ls = len(log_s)
        return loss

    @staticmethod
    def backward(ctx, g):
        z, mean, log_var, prob, lens, acc = ctx.saved_tensors
        T, B, M = z.shape
        Bm, Cn = mean.shape[0], mean.shape[2]
        dev = z.device
        g = _c(g.reshape(1).to(torch.float32))
        need = ctx.needs_input_grad
        dz = torch.empty_like(z)
        dls = torch.empty_like(z) if ctx.n_ls else None
        f32 = dict(device=dev, dtype=torch.float32)
        dmean = torch.empty(B, M, Cn, **f32) if need[1] else None
        dlv = torch.empty(B, M, Cn, **f32) if need[2] else None
        dprob = torch.empty(B, Cn, **f32) if need[3] else None
        work = None
        if need[1] or need[2] or need[3]:
            work = torch.empty(L.lib().ft_mixture_nll_work_floats(T, B, M, Cn), **f32)
        L.check(L.lib().ft_mixture_nll_bwd(L.ptr(z), L.ptr(mean), L.ptr(log_var), L.ptr(prob), L.ptr(lens), L.ptr(acc), L.ptr(g),
                                           L.ptr(dz), L.ptr(dls), L.ptr(dmean), L.ptr(dlv), L.ptr(dprob), L.ptr(work), T, B, M, Cn, Bm,
                                           L.stream()), "ft_mixture_nll_bwd")
        if Bm == 1 and B > 1:                    # shared Gaussians that ask for a gradient (the reference's are buffers): add the rows
            dmean = None if dmean is None else dmean.sum(0, keepdim=True)
            dlv = None if dlv is None else dlv.sum(0, keepdim=True)
        return (dz, dmean, dlv, dprob, None) + (dls,) * ctx.n_ls


def mixture_sample(mean, log_var, component, n_frames, sigma=1.0, rows=None, eps=None):
    """-> fp32 [S, M, n_frames]: out[s,m,t] = mean[rows[s],m,component[s]] + sigma exp(log_var[..] / 2) eps[s,m,t].  mean / log_var
    [Bm,M,C]; component int32 [S] on the device; rows int32 [S] | None (row 0, Bm = 1); eps [S,M,n_frames] | None with sigma 0."""
    mean, log_var = _c(mean.float()), _c(log_var.float())
    L.require_cuda(mean, log_var, component, rows, eps)
    Bm, M, Cn = mean.shape
    S = component.shape[0]
    if eps is not None:
        eps = _c(eps.float())
        assert tuple(eps.shape) == (S, M, n_frames)
    out = torch.empty(S, M, n_frames, device=mean.device, dtype=torch.float32)
    L.check(L.lib().ft_mixture_sample(L.ptr(mean), L.ptr(log_var), L.ptr(rows), L.ptr(component), L.ptr(eps), L.ptr(out), S, M,
                                      n_frames, Cn, Bm, float(sigma), L.stream()), "ft_mixture_sample")
    return out
