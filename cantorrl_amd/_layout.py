"""The byte layout of a step's outputs, in one place (NumPy only: no torch, no GPU).

ONE buffer holds everything a host caller reads after a step:

    [obs f32 N x 13 | reward f32 N | terminated u8 N | truncated u8 N | info fields]

with every info field 256-B aligned.  HedgingVecEnv allocates it on the device and hands the step
kernel pointers into it; step_wait copies the obs / reward / terminated prefix to the host as one
DMA, and freezing an InfoView is one device copy of the info part.  The small-N host path's mapped
block (he_host_alloc) is the same layout followed by the actions [N, 2], the terminal obs [N, 13]
and the step's completion flag (one u32), each 256-B aligned.  DeviceVecNormalize's output buffer
[obs | reward] is the layout's first `terminated` bytes; its own mapped block (host_io) is that
head followed by the normalized terminal obs and the finished episodes' Monitor sums (vn_*).
Every offset below is in bytes from the start of its buffer.
"""
import numpy as np

from ._lib import HE_OBS_DIM as D, INFO_FIELDS

ALIGN = 256
F32 = np.dtype(np.float32)


def _align(x):
    return -(-x // ALIGN) * ALIGN


class IoLayout:
    def __init__(self, n, keys=()):
        """n envs; keys: the info fields the step writes, in buffer order (KeyError for an unknown one)."""
        known = dict(INFO_FIELDS)
        self.n = n
        self.reward = n * D * 4                  # the obs start at 0
        self.terminated = self.reward + n * 4    # = the bytes of [obs | reward]
        self.truncated = self.terminated + n     # = the prefix step_wait copies (obs, reward, terminated)
        self.info0 = o = _align(self.truncated + n)
        self.fields = {}                         # key -> (dtype, offset, bytes)
        for k in keys:
            if k not in known:
                raise KeyError(f"unknown info key {k!r}")
            dt = np.dtype(known[k])
            self.fields[k] = (dt, o, n * dt.itemsize)
            o += _align(n * dt.itemsize)
        self.total = o
        # the host-mapped block
        self.actions = _align(self.total)
        self.terminal_obs = _align(self.actions + n * 2 * 4)
        self.flag = _align(self.terminal_obs + n * D * 4)   # the step's completion flag (he_step_signal)
        self.host_total = self.flag + 4
        # DeviceVecNormalize's host-mapped block (host_io): [obs | reward] as its device buffer,
        # then the normalized terminal obs [N, 13] and the finished episodes' Monitor return
        # (f64 [N]) and length (i32 [N])
        self.vn_terminal_obs = _align(self.terminated)
        self.vn_ep_ret_done = _align(self.vn_terminal_obs + n * D * 4)
        self.vn_ep_len_done = _align(self.vn_ep_ret_done + n * 8)
        self.vn_host_total = self.vn_ep_len_done + n * 4
        self._info = [(k, dt, o - self.info0, o - self.info0 + b) for k, (dt, o, b) in self.fields.items()]

    def obs_reward(self, h):
        """Host bytes [obs | reward | ...] -> (obs [n, 13], reward [n]) views."""
        return h[:self.reward].view(F32).reshape(self.n, D), h[self.reward:self.terminated].view(F32)

    def unpack(self, h):
        """Host bytes of (at least) the step prefix -> (obs [n, 13], reward [n], done bool [n]) views."""
        return (*self.obs_reward(h), h[self.terminated:self.truncated].view(np.bool_))   # the kernels store 0 / 1

    def split_info(self, flat):
        """Host bytes of the info part (from info0 on) -> {key: array} views."""
        return {k: flat[a:b].view(dt) for k, dt, a, b in self._info}

    def record_dtype(self):
        """The whole buffer as one record: obs, reward, terminated and every info field by name
        (scalars per env at n = 1, as HedgingEnv reads them; [n] columns otherwise)."""
        col = (self.n,) if self.n > 1 else ()
        names = ["obs", "reward", "terminated"] + list(self.fields)
        formats = [(F32, col + (D,)), (F32, col), ("u1", col)] + [(dt, col) for dt, _, _ in self.fields.values()]
        offsets = [0, self.reward, self.terminated] + [o for _, o, _ in self.fields.values()]
        return np.dtype({"names": names, "formats": formats, "offsets": offsets, "itemsize": self.total})

    def gather_index(self, keys):
        """Element indices of env 0's value of each of `keys` (fields of ONE dtype) in a view of the
        buffer of that dtype: buf.view(dtype)[index] reads them in one gather."""
        return np.array([self.fields[k][1] // self.fields[k][0].itemsize for k in keys], np.intp)
