"""Training / validation data from image file lists (the reference's dataset/licdataset.py and
utils/image/common.py:12-77,103-114), with the resize / crop / flip chain on the device.

Host side: file list, the random draws, and the *resize plan*: the stages the reference's crop functions would
run through PIL (BOX halvings to (w//2, h//2) while min >= 2 * smaller_dim_size, then one BICUBIC resize to
round(x * scale)), each pass with the int32 coefficient tables of Pillow's 8-bit resampling (Resample.c:
precompute_coeffs + normalize_coeffs_8bpc, computed here in float64 in Pillow's operation order). The device
kernels (csrc/image_ops.hip) evaluate those tables in integer arithmetic, so the device path equals
`Image.resize` bit for bit.

Differences from the reference, on purpose:
  * the random stream. The reference draws from Python's global `random` inside DataLoader worker processes, which
    is not reproducible (it depends on worker count and timing). Here every image's draws come from a numpy
    Generator keyed by (seed, epoch, image index): they do not depend on rank count, thread timing or resume point.
    The value ranges and the order of use are the reference's.
  * decoding runs in a thread pool of this process, never in worker processes: no process but the rank itself
    opens the GPU, nothing forks after HIP is initialised, and worker threads never call into HIP.
"""
from __future__ import annotations

import collections
import functools
import math
import queue
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

PRECISION_BITS = 22  # Pillow's 8bpc coefficient precision (32 - 8 - 2)
BOX, BICUBIC = "box", "bicubic"
_SUPPORT = {BOX: 0.5, BICUBIC: 2.0}
H_TILE = 64  # output pixels per block of the horizontal kernel (image_ops.hip H_TP)


def load_file_list(path: str) -> List[str]:
    """One path per non-empty line (utils/file.py:5-13)."""
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


# ------------------------------------------------------------------------------------------------ draws

@dataclass(frozen=True)
class CropDraws:
    smaller_dim_size: int  # target of the short side before the crop (0: crop_type none)
    crop_y: int
    crop_x: int
    hflip: bool
    vflip: bool
    rot90: bool


def image_rng(seed: int, epoch: int, index: int) -> np.random.Generator:
    return np.random.default_rng([int(seed), int(epoch), int(index)])


def resized_size(size: Tuple[int, int], smaller_dim_size: int) -> Tuple[int, int]:
    """(w, h) after the reference's halvings and BICUBIC resize."""
    for _, _, out in _stage_sizes(size, smaller_dim_size):
        size = out
    return size


def _stage_sizes(size, smaller):
    """[(filter, in (w, h), out (w, h))] exactly as center_crop_arr / random_crop_arr call Image.resize."""
    w, h = int(size[0]), int(size[1])
    out = []
    while min(w, h) >= 2 * smaller:
        out.append((BOX, (w, h), (w // 2, h // 2)))
        w, h = w // 2, h // 2
    scale = smaller / min(w, h)
    out.append((BICUBIC, (w, h), (round(w * scale), round(h * scale))))
    return out


def draw_crop(rng: np.random.Generator, size: Tuple[int, int], out_size: int, crop_type: str, use_hflip: bool,
              use_rot: bool) -> CropDraws:
    """The draws of one image, in the reference's order: smaller_dim_size, crop_y, crop_x (random_crop_arr /
    random_crop_arr_256), then hflip, vflip, rot90 (augment; a disabled flip draws nothing). `center` draws only
    the flips; `none` neither resizes nor crops."""
    if crop_type not in ("none", "center", "random"):
        raise ValueError(f"crop_type {crop_type!r}: expected none, center or random")
    smaller = cy = cx = 0
    if crop_type == "random":
        lo, hi = (0.4, 0.5) if out_size == 256 else (0.8, 1.0)  # licdataset.py:47-50
        smaller = int(rng.integers(math.ceil(out_size / hi), math.ceil(out_size / lo) + 1))
        w, h = resized_size(size, smaller)
        cy = int(rng.integers(h - out_size + 1))
        cx = int(rng.integers(w - out_size + 1))
    elif crop_type == "center":
        smaller = out_size
        w, h = resized_size(size, smaller)
        cy, cx = (h - out_size) // 2, (w - out_size) // 2
    hflip = bool(use_hflip and rng.random() < 0.5)
    vflip = bool(use_rot and rng.random() < 0.5)
    rot90 = bool(use_rot and rng.random() < 0.5)
    return CropDraws(smaller, cy, cx, hflip, vflip, rot90)


# ------------------------------------------------------------------------------------------- resize plan

def _filter(name: str, x: np.ndarray) -> np.ndarray:
    if name == BOX:
        return np.where((x > -0.5) & (x <= 0.5), 1.0, 0.0)
    a = -0.5
    x = np.abs(x)
    near = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    far = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, near, np.where(x < 2.0, far, 0.0))


@functools.lru_cache(maxsize=256)
def coeff_tables(in_size: int, out_size: int, filt: str) -> Tuple[np.ndarray, np.ndarray]:
    """(bounds int32 [out][2] = (first tap, tap count), kk int32 [out][ksize]) of one resampling axis: Pillow's
    precompute_coeffs followed by normalize_coeffs_8bpc, in float64 and in their operation order."""
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = _SUPPORT[filt] * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    k = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):  # the running sum in tap order, as the C loop
        live = x < xmax
        w = np.where(live, _filter(filt, ((x + xmin) - center + 0.5) * ss), 0.0)
        k[:, x] = w
        ww = ww + w
    nz = ww != 0.0
    k[nz] = k[nz] / ww[nz, None]
    k[np.arange(ksize)[None, :] >= xmax[:, None]] = 0.0
    kk = np.trunc(np.where(k < 0, -0.5, 0.5) + k * float(1 << PRECISION_BITS)).astype(np.int32)
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    bounds.setflags(write=False)
    kk.setflags(write=False)
    return bounds, kk


@dataclass(frozen=True)
class Pass:
    axis: str            # "h": along x (runs first, uint8 intermediate), "v": along y
    in_size: int
    out_size: int
    bounds: np.ndarray   # int32 [out_size][2]
    kk: np.ndarray       # int32 [out_size][ksize]

    @property
    def ksize(self) -> int:
        return self.kk.shape[1]

    @functools.cached_property
    def seg_max(self) -> int:
        """The most source pixels any H_TILE consecutive outputs read (the horizontal kernel's LDS segment)."""
        first = self.bounds[:, 0].astype(np.int64)
        end = first + self.bounds[:, 1]
        last = np.minimum(np.arange(self.out_size) + H_TILE - 1, self.out_size - 1)
        return int(np.max(end[last] - first))


@dataclass(frozen=True)
class Stage:
    filter: str
    in_size: Tuple[int, int]   # (w, h)
    out_size: Tuple[int, int]
    passes: Tuple[Pass, ...]


@functools.lru_cache(maxsize=512)
def resize_plan(size: Tuple[int, int], smaller_dim_size: int) -> Tuple[Stage, ...]:
    """The stages the reference's crop functions run for a (w, h) image. A stage whose output size equals its
    input size is dropped (Image.resize returns a copy there), and so is a pass along an axis that keeps its size
    (ImagingResample's need_horizontal / need_vertical)."""
    stages = []
    for filt, (w, h), (ow, oh) in _stage_sizes(size, smaller_dim_size):
        if (ow, oh) == (w, h):
            continue
        passes = []
        if ow != w:
            passes.append(Pass("h", w, ow, *coeff_tables(w, ow, filt)))
        if oh != h:
            passes.append(Pass("v", h, oh, *coeff_tables(h, oh, filt)))
        stages.append(Stage(filt, (w, h), (ow, oh), tuple(passes)))
    return tuple(stages)


def plan_tables(plan: Sequence[Stage]) -> Tuple[np.ndarray, List[Tuple[int, int]]]:
    """Every pass's tables as one int32 array, and (bounds offset, kk offset) per pass in plan order."""
    parts, offs, n = [], [], 0
    for st in plan:
        for p in st.passes:
            offs.append((n, n + p.bounds.size))
            parts += [p.bounds.ravel(), p.kk.ravel()]
            n += p.bounds.size + p.kk.size
    return (np.concatenate(parts) if parts else np.zeros(0, np.int32)), offs


# ------------------------------------------------------------------------------------- the chain on the host

def check_passthrough(size: Tuple[int, int]) -> None:
    if size[0] % 64 or size[1] % 64:
        raise ValueError(f"crop_type none passes images through: their sides must be multiples of 64, got "
                         f"{size[0]}x{size[1]}")


def process_host(img, d: CropDraws, out_size: int, crop_type: str) -> np.ndarray:
    """The reference chain through PIL (the fallback path and the A/B baseline): uint8 HWC."""
    from PIL import Image
    if crop_type == "none":
        check_passthrough(img.size)
        arr = np.array(img)
    else:
        for filt, _, out in _stage_sizes(img.size, d.smaller_dim_size):
            img = img.resize(out, resample=Image.BOX if filt == BOX else Image.BICUBIC)
        arr = np.array(img)[d.crop_y:d.crop_y + out_size, d.crop_x:d.crop_x + out_size]
    return np.ascontiguousarray(flip_host(arr, d))


def flip_host(arr: np.ndarray, d: CropDraws) -> np.ndarray:
    if d.hflip:
        arr = arr[:, ::-1]
    if d.vflip:
        arr = arr[::-1]
    if d.rot90:
        arr = arr.transpose(1, 0, 2)
    return arr


# ----------------------------------------------------------------------------------- the chain on the device

def _r4(n: int) -> int:
    return (n + 3) & ~3


def process_device(raw: torch.Tensor, size: Tuple[int, int], stride: int, tables: torch.Tensor,
                   offs: Sequence[Tuple[int, int]], plan: Sequence[Stage], d: CropDraws, out_size: int,
                   crop_type: str, dst: torch.Tensor, stream: int,
                   window: Optional[Tuple[int, int, int, int]] = None) -> None:
    """Run `plan`, the crop and the flips of one image on `stream` and write dst ([oh, ow, 3] uint8, dense: one
    image's slot of the batch). raw: the image's bytes on the device, rows `stride` bytes apart; tables: the
    device copy of plan_tables(plan)[0]. Every stage but the last is computed whole; the last computes only the
    crop window, and its horizontal pass only the rows the vertical one reads. `window` (y, x, h, w) replaces the
    out_size square at the draws' offsets."""
    from ._lib import call
    w, h = size
    if window is not None:
        win = tuple(int(v) for v in window)
    elif crop_type == "none":
        win = (0, 0, h, w)
    else:
        win = (d.crop_y, d.crop_x, out_size, out_size)
    fw, fh = plan[-1].out_size if plan else (w, h)
    if min(win) < 0 or win[2] < 1 or win[3] < 1 or win[0] + win[2] > fh or win[1] + win[3] > fw:
        raise ValueError(f"window {win} (y, x, h, w) does not lie in the {fw}x{fh} resized image")
    want = (win[3], win[2], 3) if d.rot90 else (win[2], win[3], 3)
    if tuple(dst.shape) != want or not dst.is_contiguous() or dst.dtype != torch.uint8:
        raise ValueError(f"dst must be a dense uint8 {want}, got {tuple(dst.shape)} strides {dst.stride()}")
    src, keep, pi = raw, [raw], 0
    tbase = tables.data_ptr()
    for si, st in enumerate(plan):
        last = si == len(plan) - 1
        (iw, ih), (ow, oh) = st.in_size, st.out_size
        cy, cx, wh, ww = win if last else (0, 0, oh, ow)
        hp = next((p for p in st.passes if p.axis == "h"), None)
        vp = next((p for p in st.passes if p.axis == "v"), None)
        r0, r1 = cy, cy + wh  # source rows the stage reads
        if vp is not None:
            r0 = int(vp.bounds[cy, 0])
            r1 = int(vp.bounds[cy + wh - 1, 0] + vp.bounds[cy + wh - 1, 1])
        cb0 = cx * 3  # first byte column of `src` the vertical pass reads
        if hp is not None:
            bo, ko = offs[pi]
            pi += 1
            tmp = torch.empty((r1 - r0, _r4(ww * 3)), dtype=torch.uint8, device=raw.device)
            call("rdeic_resample_h_u8", src.data_ptr(), stride, ih, iw, tbase + 4 * bo, tbase + 4 * ko, hp.ksize, ow,
                 hp.seg_max, r0, r1 - r0, cx, ww, tmp.data_ptr(), tmp.stride(0), stream)
            src, stride, row0, cb0 = tmp, tmp.stride(0), r0, 0
            keep.append(tmp)
        else:
            row0 = 0
        if vp is not None:
            bo, ko = offs[pi]
            pi += 1
            src_rows = (r1 - r0) if hp is not None else ih
            row_bytes = ww * 3 if hp is not None else iw * 3
            tmp = torch.empty((wh, _r4(ww * 3)), dtype=torch.uint8, device=raw.device)
            call("rdeic_resample_v_u8", src.data_ptr(), stride, row_bytes, row0, src_rows, tbase + 4 * bo,
                 tbase + 4 * ko, vp.ksize, oh, cy, wh, cb0, ww * 3, tmp.data_ptr(), tmp.stride(0), stream)
            src, stride = tmp, tmp.stride(0)
            keep.append(tmp)
        if last:  # src now holds exactly the window
            w, h, win = ww, wh, (0, 0, wh, ww)
        else:
            w, h = ow, oh
    call("rdeic_crop_flip_u8", src.data_ptr(), stride, h, w, win[0], win[1], win[2], win[3], int(d.hflip),
         int(d.vflip), int(d.rot90), dst.data_ptr(), stream)


# ------------------------------------------------------------------------------------------------ loader

class _Slot:
    """One pinned staging buffer (allocated and grown on the consumer thread only)."""

    def __init__(self, cap: int):
        self.pin = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        self.np = self.pin.numpy()
        self.cap = cap


@dataclass
class _Item:
    index: int
    draws: CropDraws
    size: Tuple[int, int]
    arr: Optional[np.ndarray] = None    # the decoded (or host-resized) image when it is not in a slot
    slot: Optional[_Slot] = None
    stride: int = 0
    nbytes: int = 0                     # bytes of the slot in use (image, then tables)
    tab_off: int = 0
    plan: Tuple[Stage, ...] = ()
    offs: Sequence[Tuple[int, int]] = ()
    tables: Optional[np.ndarray] = None


def open_rgb(path: str):
    """Image.open(path).convert("RGB"), three attempts (licdataset.py:35-42)."""
    from PIL import Image
    err = None
    for attempt in range(3):
        try:
            return Image.open(path).convert("RGB")
        except Exception as e:  # the reference retries on anything
            err = e
            if attempt < 2:
                time.sleep(1)
    raise RuntimeError(f"failed to load image {path}: {err}")


class ImageListLoader:
    """Batches of uint8 [B, S, S, 3] on `device` from an image file list, the form FineTuner.training_step takes.

    PIL decodes on a thread pool sized like the host coders' (coders.default_threads(): the cgroup CPU quota
    divided by LOCAL_WORLD_SIZE, never os.cpu_count()). A worker writes the decoded HWC bytes and the plan's
    tables into a pinned staging buffer; the consumer thread copies them across on a side stream, runs the
    device chain there and makes the current stream wait on an event. host_resize=True runs the same chain
    through PIL on the workers instead (the fallback and the A/B baseline; the only mode with a CPU device).

    Epoch order is a permutation seeded by (seed, epoch) (the identity without shuffle); rank r takes positions
    r, r + world, ...; drop_last as torch's DataLoader. seek(global_step) positions the loader where an
    uninterrupted run would be after that many batches, decoding nothing.
    """

    def __init__(self, file_list, out_size: int, crop_type: str, use_hflip: bool, use_rot: bool, batch_size: int,
                 shuffle: bool, drop_last: bool, seed: int, rank: int = 0, world: int = 1, device="cuda",
                 threads: Optional[int] = None, prefetch: int = 2, host_resize: bool = False):
        self.paths = load_file_list(file_list) if isinstance(file_list, str) else list(file_list)
        if crop_type not in ("none", "center", "random"):
            raise ValueError(f"crop_type {crop_type!r}: expected none, center or random")
        self.out_size, self.crop_type = int(out_size), crop_type
        self.use_hflip, self.use_rot = bool(use_hflip), bool(use_rot)
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), bool(shuffle), bool(drop_last)
        self.seed, self.rank, self.world = int(seed), int(rank), int(world)
        self.device = torch.device(device)
        self.host_resize = bool(host_resize)
        if self.device.type != "cuda" and not self.host_resize:
            raise ValueError("the device resize path needs a GPU device; pass host_resize=True for CPU tensors")
        if threads is None:
            from .coders import default_threads
            threads = default_threads()
        self.threads = max(1, int(threads))
        self.prefetch = max(1, int(prefetch))
        n_mine = len(range(self.rank, len(self.paths), self.world))
        self.batches_per_epoch = n_mine // self.batch_size if self.drop_last else -(-n_mine // self.batch_size)
        if self.batches_per_epoch == 0:
            raise ValueError(f"{len(self.paths)} images over {self.world} ranks give rank {self.rank} no batch of "
                             f"{self.batch_size}")
        self.epoch, self.pos = 0, 0
        self._pool = ThreadPoolExecutor(self.threads, thread_name_prefix="rdeic-decode")
        self._free: "queue.Queue[_Slot]" = queue.Queue()
        self._nslots = 0
        self._cap = max(self.out_size * self.out_size * 3, 1 << 22)
        self._side = None
        self._busy = collections.deque()  # (event, slots) of batches whose copies may still be in flight

    def __len__(self) -> int:
        return self.batches_per_epoch

    def close(self) -> None:
        self._pool.shutdown(wait=True, cancel_futures=True)

    # -- order
    def epoch_indices(self, epoch: int) -> np.ndarray:
        """This rank's image indices of `epoch`, in order."""
        n = len(self.paths)
        order = np.random.default_rng([self.seed, int(epoch)]).permutation(n) if self.shuffle else np.arange(n)
        return order[self.rank::self.world]

    def batch_indices(self, epoch: int, pos: int) -> np.ndarray:
        mine = self.epoch_indices(epoch)
        return mine[pos * self.batch_size:(pos + 1) * self.batch_size]

    def seek(self, global_step: int) -> None:
        self.epoch, self.pos = divmod(int(global_step), self.batches_per_epoch)

    # -- worker side (no HIP calls here)
    def _load(self, index: int, epoch: int) -> _Item:
        img = open_rgb(self.paths[index])
        size = img.size
        d = draw_crop(image_rng(self.seed, epoch, index), size, self.out_size, self.crop_type, self.use_hflip,
                      self.use_rot)
        if self.host_resize:
            arr = process_host(img, d, self.out_size, self.crop_type)
            it = _Item(index, d, size, arr=arr, nbytes=arr.size)
            if self.device.type == "cuda":
                slot = self._free.get()
                if slot.cap >= arr.size:
                    slot.np[:arr.size] = arr.reshape(-1)
                    it.arr = None
                it.slot = slot
            return it
        if self.crop_type == "none":
            check_passthrough(size)
        plan = resize_plan(size, d.smaller_dim_size) if self.crop_type != "none" else ()
        tables, offs = plan_tables(plan)
        w, h = size
        stride = _r4(w * 3)
        tab_off = (h * stride + 15) & ~15
        it = _Item(index, d, size, stride=stride, nbytes=tab_off + tables.nbytes, tab_off=tab_off, plan=plan,
                   offs=offs, tables=tables)
        arr = np.asarray(img).reshape(h, w * 3)
        slot = it.slot = self._free.get()
        if slot.cap >= it.nbytes:
            self._fill(slot, it, arr)
        else:
            it.arr = arr  # the consumer grows the slot
        return it

    @staticmethod
    def _fill(slot: _Slot, it: _Item, arr: np.ndarray) -> None:
        h, wb = arr.shape
        slot.np[:h * it.stride].reshape(h, it.stride)[:, :wb] = arr
        slot.np[it.tab_off:it.nbytes].view(np.int32)[:] = it.tables

    # -- consumer side
    def _ensure_slots(self) -> None:
        if self.device.type != "cuda":
            return
        if self._side is None:
            self._side = torch.cuda.Stream(self.device)
        want = self.batch_size * (self.prefetch + 1)
        while self._nslots < want:
            self._free.put(_Slot(self._cap))
            self._nslots += 1

    def _release(self, keep: int) -> None:
        while len(self._busy) > keep:
            ev, slots = self._busy.popleft()
            ev.synchronize()
            for s in slots:
                self._free.put(s)

    def _assemble(self, items: List[_Item]) -> torch.Tensor:
        shapes = {(i.arr.shape if self.host_resize and i.arr is not None else self._out_shape(i)) for i in items}
        if len(shapes) != 1:
            self._give_back(items)
            raise ValueError(f"crop_type none passes images through: the images of a batch must have equal sides, "
                             f"got {sorted(shapes)}")
        shape = next(iter(shapes))
        if self.device.type != "cuda":
            return torch.from_numpy(np.stack([i.arr for i in items]))
        self._release(0)
        cur = torch.cuda.current_stream(self.device)
        slots = []
        with torch.cuda.stream(self._side):
            out = torch.empty((len(items),) + tuple(shape), dtype=torch.uint8, device=self.device)
            for b, it in enumerate(items):
                slot = it.slot
                if it.arr is not None:  # did not fit: a larger slot replaces this one
                    self._cap = max(self._cap, 1 << (it.nbytes - 1).bit_length())
                    slot = _Slot(self._cap)
                    if self.host_resize:
                        slot.np[:it.nbytes] = it.arr.reshape(-1)
                    else:
                        self._fill(slot, it, it.arr)
                slots.append(slot)
                if self.host_resize:
                    out[b].view(-1).copy_(slot.pin[:it.nbytes], non_blocking=True)
                    continue
                raw = torch.empty(it.nbytes, dtype=torch.uint8, device=self.device)
                raw.copy_(slot.pin[:it.nbytes], non_blocking=True)
                process_device(raw, it.size, it.stride, raw[it.tab_off:].view(torch.int32), it.offs, it.plan,
                               it.draws, self.out_size, self.crop_type, out[b], self._side.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(self._side)
        cur.wait_event(ev)
        out.record_stream(cur)
        self._busy.append((ev, slots))
        return out

    def _give_back(self, items) -> None:
        for it in items:
            if it.slot is not None:
                self._free.put(it.slot)

    def _collect(self, futs) -> List[_Item]:
        """The futures' items; if a load failed, the slots of the others go back before the error is raised."""
        items, err = [], None
        for f in futs:
            try:
                items.append(f.result())
            except Exception as e:
                err = err or e
        if err is not None:
            self._give_back(items)
            raise err
        return items

    def _out_shape(self, it: _Item) -> Tuple[int, int, int]:
        if self.crop_type == "none":
            w, h = it.size
        else:
            w = h = self.out_size
        return (w, h, 3) if it.draws.rot90 else (h, w, 3)

    def _positions(self, forever: bool):
        epoch, pos = self.epoch, self.pos
        while True:
            while pos < self.batches_per_epoch:
                yield epoch, pos
                pos += 1
            epoch, pos = epoch + 1, 0
            if not forever:
                return

    def _run(self, forever: bool):
        self._ensure_slots()
        pending = collections.deque()
        positions = self._positions(forever)
        try:
            while True:
                while len(pending) < self.prefetch:
                    nxt = next(positions, None)
                    if nxt is None:
                        break
                    e, p = nxt
                    pending.append((e, p, [self._pool.submit(self._load, int(i), e)
                                           for i in self.batch_indices(e, p)]))
                if not pending:
                    break
                e, p, futs = pending.popleft()
                batch = self._assemble(self._collect(futs))
                self.epoch, self.pos = (e, p + 1) if p + 1 < self.batches_per_epoch else (e + 1, 0)
                yield batch
        finally:
            for _, _, futs in pending:  # hand the slots of abandoned prefetches back
                for f in futs:
                    if not f.cancel():
                        try:
                            self._give_back([f.result()])
                        except Exception:
                            pass
            if self.device.type == "cuda":
                self._release(0)

    def load_batch(self, indices: Sequence[int], epoch: int = 0) -> torch.Tensor:
        """The batch of the given image indices under epoch's draws (the Validator walks its shard with it)."""
        if not 0 < len(indices) <= self.batch_size:
            raise ValueError(f"load_batch takes 1 to batch_size = {self.batch_size} indices, got {len(indices)}")
        self._ensure_slots()
        futs = [self._pool.submit(self._load, int(i), int(epoch)) for i in indices]
        return self._assemble(self._collect(futs))

    def __iter__(self):
        """One epoch from the current position (the start, or where seek() put it)."""
        return self._run(False)

    def forever(self):
        """Batches across epochs without end (train.py steps by max_steps)."""
        return self._run(True)
