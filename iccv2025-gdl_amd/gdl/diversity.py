"""The feature-diversity monitor of the reference's main.py (get_feature_diversity, :77-89) on the device: csrc/diversity.hip
behind gdl_feature_diversity.  Per image, with x_p the 512 channels at position p of a [512, h, w] map (P = h w):

    c_p = x_p - mean(x_p),  s_p = std(x_p) (unbiased),  R_pq = (c_p . c_q) / (s_p s_q),  d = ||R||_F / P^2

and the value is the mean of d over the images -- what main.py:183-184 computes with two bmm, a std, a norm and a host sync
per encoder and step.  A position whose channels are all equal gives NaN (the script's 0 / 0), never Inf.
"""
from collections import OrderedDict

import torch

from . import _lib as L

# (device index, stream handle) -> zeroed workspace (ticket counter + per-image terms), grown on demand: launches sharing one
# must be ordered on one stream.  The _WS_MAX most recently used are kept, so short-lived streams cannot make it grow; a dropped
# one goes back to the caching allocator, which hands it out again only behind the work of the stream it was allocated on.
_WS = OrderedDict()
_WS_MAX = 8


def workspace(n_img, device):
    """A zeroed gdl_feature_diversity workspace for `n_img` images (every launch leaves it zeroed where it matters)."""
    return torch.zeros(L.load().gdl_feature_diversity_workspace_bytes(n_img), dtype=torch.uint8, device=device)


def feature_diversity(fmap, per_image=False):
    """main.py's get_feature_diversity of an encoder's final feature map `fmap` [N, 512, h, w] (h w <= 256) on the device:
    a contiguous float32 tensor (NCHW, what the drop-in encoders return) or a channels-last float32 / bfloat16 tensor -- read
    where it lies, no copy.  Returns a 0-dim float32 device tensor (with per_image=True: that and the [N] per-image values),
    enqueued on the current stream without a host sync.  float32 arithmetic whatever the storage type.  A host tensor raises:
    there is no CPU path."""
    if not isinstance(fmap, torch.Tensor) or fmap.device.type != "cuda":
        raise L.GdlError("gdl.feature_diversity: the map must be a tensor on an MI355X (cuda) device; there is no CPU path")
    if fmap.dim() != 4 or fmap.shape[0] < 1 or fmap.shape[2] * fmap.shape[3] < 1:
        raise L.GdlError(f"gdl.feature_diversity: the map must be [N, 512, h, w], got {tuple(fmap.shape)}")
    N, C, h, w = fmap.shape
    if fmap.dtype == torch.float32 and fmap.is_contiguous():
        dt, layout = L.GDL_F32, L.GDL_LAYOUT_NCHW
    elif fmap.dtype in (torch.float32, torch.bfloat16) and fmap.is_contiguous(memory_format=torch.channels_last):
        dt, layout = (L.GDL_BF16 if fmap.dtype == torch.bfloat16 else L.GDL_F32), L.GDL_LAYOUT_NHWC
    else:
        raise L.GdlError("gdl.feature_diversity: the map must be contiguous float32 (NCHW) or channels-last float32 / bfloat16; "
                         f"got {fmap.dtype}, strides {tuple(fmap.stride())}")
    with torch.cuda.device(fmap.device):
        st = L.cur_stream()  # the map's device's current stream
        key = (fmap.device.index, st)
        ws = _WS.get(key)
        if ws is None or ws.numel() < L.load().gdl_feature_diversity_workspace_bytes(N):
            ws = _WS[key] = workspace(max(N, 256), fmap.device)
        _WS.move_to_end(key)
        while len(_WS) > _WS_MAX:
            _WS.popitem(last=False)
        out = torch.empty(1, device=fmap.device)
        per = torch.empty(N, device=fmap.device) if per_image else None
        L.call("gdl_feature_diversity", fmap.data_ptr(), dt, layout, N, h * w, C, L.ptr(per), L.ptr(out), None, L.ptr(ws),
               ws.numel(), st)
    return (out[0], per) if per_image else out[0]
