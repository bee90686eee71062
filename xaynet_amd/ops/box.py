"""Batched NaCl boxes on the GPU (K8): XSalsa20-Poly1305 over many
independent messages in one launch, byte for byte what `_core.crypto` (and
libsodium) produce.

A batch lives in one packed device buffer. Every box gets `_HEAD` bytes of
head room and its message starts on a 64-byte boundary, so the kernels' 16-byte
accesses are aligned, the tag (and a sealed box's ephemeral key) sit right in
front of the ciphertext, and an opened payload is a 16-byte-aligned view that a
later kernel can read in place. By default X25519 and the sealed-box nonce
(blake2b) stay on the host and only the bulk pass over the bytes runs on the
device; `device_keys=True` moves them to the device as well (K9: one Montgomery
ladder per lane, then HSalsa20 and the nonce per box), and `open_seeds` /
`seal_seed` are the seed-dict forms of that path.

The kernels decrypt and authenticate in one pass, so plaintext of a forged
box does exist in the output buffer for a moment: a last kernel zeroes it, and
this layer hands out `None` for it. Nothing here returns a view of a box whose
tag failed.
"""
from __future__ import annotations

import numpy as np
import torch

from xaynet_amd import _core

from .engine import _hip, _require_gpu

_OPEN, _SEAL, _MAC = 0, 1, 2
_HEAD = 64  # bytes in front of every message: room for epk(32) || tag(16)
_crypto = _core.crypto
_BASE_POINT = bytes([9]) + bytes(31)


def _nbytes(item):
    """Bytes of a host buffer or a device tensor of any dtype."""
    if isinstance(item, torch.Tensor):
        return item.numel() * item.element_size()
    return memoryview(item).nbytes


def _as_bytes(t):
    """A device tensor of any dtype as a flat uint8 tensor."""
    return t.contiguous().view(torch.uint8).reshape(-1)


def _layout(lens):
    """Message offsets of a batch and the packed buffer's size."""
    offs, at = [], 0
    for n in lens:
        offs.append(at + _HEAD)
        at += _HEAD + (n + 63) // 64 * 64
    return offs, at + _HEAD


def chunk_sets(entries):
    """Group the messages of a batch into complete updates by the multipart
    rule of Coordinator::handle_message_bytes, applied message by message in
    batch order. entries[i] is (participant pk, tag, multipart flag, chunk id,
    message id, last flag, data length) of a message whose header signature
    verified. Returns (sets, host_sets, pending): every complete set as the
    list of its entry indices in chunk order, in order of completion; of those,
    the multipart sets whose chunk 0 carries fewer than 136 data bytes (its
    task signatures straddle chunks) apart in host_sets; and the indices, in
    batch order, of the chunks whose set is still open at the end. A message
    that is no chunk is a set of one. The key of a set is (pk, message id); a
    duplicate id overwrites the earlier chunk; two different last ids corrupt
    the set, as do ids other than 0..last once last + 1 chunks are there, and a
    corrupt set's chunks appear nowhere; chunks behind a completion start a
    new set."""
    sets, host_sets, open_sets = [], [], {}
    for i, (pk, _tag, multipart, cid, mid, last, _n) in enumerate(entries):
        if not multipart:
            sets.append([i])
            continue
        key = (bytes(pk), mid)
        chunks, last_id = open_sets.get(key, ({}, -1))
        chunks[cid] = i
        if last:
            if last_id >= 0 and last_id != cid:
                open_sets.pop(key, None)
                continue
            last_id = cid
        open_sets[key] = (chunks, last_id)
        if last_id >= 0 and len(chunks) == last_id + 1:
            del open_sets[key]
            if sorted(chunks) == list(range(last_id + 1)):
                done = [chunks[c] for c in range(last_id + 1)]
                (sets if entries[done[0]][6] >= 136 else host_sets).append(done)
    pending = sorted(i for chunks, _ in open_sets.values() for i in chunks.values())
    return sets, host_sets, pending


class GpuBox:
    """Seal and open batches of boxes on one GPU. `kernel_ms` is the device
    time of the last batch's kernels when `time_kernels` is set. After an
    open, `opened_buffer` is the packed uint8 device buffer the returned views
    lie in and `opened_offsets[i]` the byte offset of box i's payload in it
    (a multiple of 16; None for a box shorter than a tag): the payload of a
    box that failed is zeros there."""

    def __init__(self, device: str = "cuda:0", time_kernels: bool = False):
        _require_gpu()
        self.device = torch.device(device)
        self.time_kernels = time_kernels
        self.kernel_ms = None
        self._pin = None  # pinned staging buffer, grown on demand, wiped after a seal
        self.opened_buffer = self.opened_offsets = None
        self._work = None
        self._up = None  # pinned descriptors and scalars of a sealed-box run, wiped by each

    # ---------------- packing ----------------

    def _new(self, nbytes):
        return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)

    def _pack(self, items, offs, front, total, wipe=False):
        """The items (host buffers or device tensors) in one device buffer,
        item i starting `front` bytes before offs[i]. Host items go through
        one pinned staging buffer and one copy; `wipe` zeroes what they left
        there (plaintext on its way to a seal) once it is on the device."""
        buf = self._new(total)
        host = [i for i, it in enumerate(items) if not isinstance(it, torch.Tensor)]
        if host:
            if self._pin is None or self._pin.numel() < total:
                self._pin = torch.empty(total, dtype=torch.uint8).pin_memory()
            stage = self._pin.numpy()
            for i in host:
                view = np.frombuffer(memoryview(items[i]).cast("B"), dtype=np.uint8)
                stage[offs[i] - front:offs[i] - front + view.size] = view
            if len(host) == len(items):
                buf.copy_(self._pin[:total])
            else:
                for i in host:
                    a, b = offs[i] - front, offs[i] - front + _nbytes(items[i])
                    buf[a:b].copy_(self._pin[a:b])
            if wipe:  # the copies above block until the bytes have left
                self._pin[:total].zero_()
        for i, it in enumerate(items):
            if isinstance(it, torch.Tensor):
                flat = _as_bytes(it.to(self.device))
                buf[offs[i] - front:offs[i] - front + flat.numel()].copy_(flat)
        return buf

    def _run(self, mode, lens, keys, nonces, src, src_offs, dst, dst_offs):
        keys = [bytes(k) for k in keys]
        nonces = [bytes(n) for n in nonces]
        if len(keys) != len(lens) or any(len(k) != 32 for k in keys):
            raise ValueError("one 32-byte key a box")
        if mode != _MAC and (len(nonces) != len(lens) or any(len(n) != 24 for n in nonces)):
            raise ValueError("one 24-byte nonce a box")
        with torch.cuda.device(self.device):
            _, work_bytes = _hip._box_plan(lens)
            if self._work is None or self._work.numel() < work_bytes:
                self._work = self._new(work_bytes)
            ok = torch.empty(len(lens), dtype=torch.int32, device=self.device)
            if self.time_kernels:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
            _hip._box_run(mode, b"".join(keys), b"".join(nonces), lens, src_offs, dst_offs,
                          src.data_ptr(), src.numel(), dst.data_ptr(), dst.numel(),
                          self._work.data_ptr(), self._work.numel(), ok.data_ptr())
            if self.time_kernels:
                t1.record()
                t1.synchronize()
                self.kernel_ms = t0.elapsed_time(t1)
        return ok

    def _run_sealed(self, mode, lens, sk, pks, src, src_offs, dst, dst_offs):
        """K9 then K8: as _run, the keys and nonces derived on the device.
        sk: the recipient's secret key (open); a seal's ephemeral secret keys
        are drawn here. pks: 32 bytes, or 32 a box (seal)."""
        n = len(lens)
        with torch.cuda.device(self.device):
            work_bytes, up_bytes, ladders_off = _hip._sealbox_plan(mode, lens)
            if self._work is None or self._work.numel() < work_bytes:
                self._work = self._new(work_bytes)
            if self._up is None or self._up.numel() < up_bytes:
                self._up = torch.empty(up_bytes, dtype=torch.uint8).pin_memory()
            ok = torch.empty(n, dtype=torch.int32, device=self.device)
            if mode == _SEAL:
                # the host's randombytes, straight into the scalars of the
                # ladder rows: the pinned upload buffer holds the only host
                # copy, and the binding zeroes that buffer after the upload
                rows = self._up.numpy()[ladders_off:ladders_off + 64 * n].reshape(n, 64)
                _crypto.randombytes_into(rows[:, :32])
            if self.time_kernels:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
            _hip._sealbox_run(mode, self._up.data_ptr(), self._up.numel(), sk, pks, lens,
                              src_offs, dst_offs, src.data_ptr(), src.numel(), dst.data_ptr(),
                              dst.numel(), self._work.data_ptr(), self._work.numel(),
                              ok.data_ptr())
            if self.time_kernels:
                t1.record()
                t1.synchronize()
                self.kernel_ms = t0.elapsed_time(t1)
        return ok

    # ---------------- X25519 ----------------

    def x25519_batch(self, scalars, points=None):
        """X25519(scalar, point) of every pair on the device, one ladder per
        lane (K9); `points=None` is the base point. Returns 32-byte values. No
        low-order-point rejection: such a point gives 32 zero bytes, as
        `_core.crypto.x25519` does."""
        scalars = [bytes(s) for s in scalars]
        points = [_BASE_POINT] * len(scalars) if points is None else [bytes(p) for p in points]
        if len(points) != len(scalars) or any(len(v) != 32 for v in scalars + points):
            raise ValueError("one 32-byte scalar and one 32-byte point a ladder")
        if not scalars:
            return []
        with torch.cuda.device(self.device):
            if self._work is None or self._work.numel() < 64 * len(scalars):
                self._work = self._new(64 * len(scalars))
            out = _hip._x25519_batch(b"".join(scalars), b"".join(points), self._work.data_ptr(),
                                     self._work.numel())
        return [out[32 * i:32 * i + 32] for i in range(len(scalars))]

    # ---------------- secretbox ----------------

    def secretbox_open_batch(self, boxes, keys, nonces):
        """Open tag || cipher boxes. Returns (messages, ok): message i is a
        uint8 device view into one packed buffer, or None where the tag failed
        (or the box is shorter than a tag); ok is the device bool tensor."""
        n = len(boxes)
        live = [i for i in range(n) if _nbytes(boxes[i]) >= 16]
        ok = torch.zeros(n, dtype=torch.bool, device=self.device)
        out = [None] * n
        self.opened_buffer, self.opened_offsets = None, [None] * n
        if not live:
            return out, ok
        lens = [_nbytes(boxes[i]) - 16 for i in live]
        offs, total = _layout(lens)
        src = self._pack([boxes[i] for i in live], offs, 16, total)
        dst = self._new(total)
        good = self._run(_OPEN, lens, [keys[i] for i in live], [nonces[i] for i in live], src,
                         offs, dst, offs).bool()
        return self._opened(out, ok, live, offs, lens, dst, good)

    def _opened(self, out, ok, live, offs, lens, dst, good):
        """What an open hands back: views of the boxes whose tag matched."""
        ok[torch.tensor(live, device=self.device)] = good
        self.opened_buffer = dst
        for i, off, m, g in zip(live, offs, lens, good.tolist()):
            self.opened_offsets[i] = off
            if g:
                out[i] = dst[off:off + m]
        return out, ok

    def _seal(self, messages, keys, nonces, heads=None):
        lens = [_nbytes(m) for m in messages]
        offs, total = _layout(lens)
        src = self._pack(messages, offs, 0, total, wipe=True)
        dst = self._new(total)
        self._run(_SEAL, lens, keys, nonces, src, offs, dst, offs)
        front = 16
        if heads is not None:  # epk in front of every tag
            front = 48
            at = torch.tensor(offs, device=self.device)[:, None] - 48 + \
                torch.arange(32, device=self.device)
            epk = torch.frombuffer(bytearray(b"".join(heads)), dtype=torch.uint8)
            dst[at.reshape(-1)] = epk.to(self.device)
        return [dst[off - front:off + m] for off, m in zip(offs, lens)]

    def secretbox_seal_batch(self, messages, keys, nonces):
        """Seal host buffers or device tensors; returns uint8 device tensors
        tag || cipher, views into one packed buffer."""
        if not len(messages):
            return []
        return self._seal(messages, keys, nonces)

    # ---------------- sealed boxes ----------------

    def sealbox_open_batch(self, sealed, pk, sk, device_keys=False):
        """Open epk || tag || cipher sealed boxes addressed to (pk, sk): as
        secretbox_open_batch, with the key agreement per box on the host, or,
        with `device_keys`, on the device: no host ladder and no read back of
        a device input's ephemeral key."""
        pk, sk = bytes(pk), bytes(sk)
        if device_keys:
            return self._sealbox_open_device(sealed, pk, sk)
        boxes, keys, nonces = [], [], []
        for s in sealed:
            if isinstance(s, torch.Tensor):
                s = _as_bytes(s)
            if _nbytes(s) < 48:
                boxes.append(b"")
                keys.append(bytes(32))
                nonces.append(bytes(24))
                continue
            epk = bytes(s[:32].cpu().numpy()) if isinstance(s, torch.Tensor) else \
                bytes(memoryview(s).cast("B")[:32])
            boxes.append(s[32:] if isinstance(s, torch.Tensor) else memoryview(s).cast("B")[32:])
            keys.append(_crypto.box_beforenm(epk, sk))
            nonces.append(_crypto.blake2b(epk + pk, 24))
        return self.secretbox_open_batch(boxes, keys, nonces)

    def _sealbox_open_device(self, sealed, pk, sk):
        if len(pk) != 32 or len(sk) != 32:
            raise ValueError("keys are 32 bytes")
        n = len(sealed)
        live = [i for i in range(n) if _nbytes(sealed[i]) >= 48]
        ok = torch.zeros(n, dtype=torch.bool, device=self.device)
        out = [None] * n
        self.opened_buffer, self.opened_offsets = None, [None] * n
        if not live:
            return out, ok
        lens = [_nbytes(sealed[i]) - 48 for i in live]
        offs, total = _layout(lens)
        src = self._pack([sealed[i] for i in live], offs, 48, total)
        dst = self._new(total)
        good = self._run_sealed(_OPEN, lens, sk, pk, src, offs, dst, offs).bool()
        return self._opened(out, ok, live, offs, lens, dst, good)

    def sealbox_seal_batch(self, messages, pk, device_keys=False):
        """Seal to pk with a fresh ephemeral key per message; returns uint8
        device tensors epk || tag || cipher. With `device_keys`, pk is one key
        or one key per message, and the ephemeral secret keys (32 bytes a box
        from the host's randombytes) go up once with the descriptors: both
        ladders of a box, its key and its nonce are computed on the device."""
        if not len(messages):
            return []
        if device_keys:
            dst, offs, lens = self._sealbox_seal_device(messages, pk)
            return [dst[off - 48:off + m] for off, m in zip(offs, lens)]
        pk = bytes(pk)
        heads, keys, nonces = [], [], []
        for _ in messages:
            epk, esk = _crypto.box_keypair()
            heads.append(epk)
            keys.append(_crypto.box_beforenm(pk, esk))
            nonces.append(_crypto.blake2b(epk + pk, 24))
        return self._seal(messages, keys, nonces, heads)

    def _sealbox_seal_device(self, messages, pk):
        one = isinstance(pk, (bytes, bytearray, memoryview))
        pks = bytes(pk) if one else b"".join(bytes(k) for k in pk)
        if len(pks) != (32 if one else 32 * len(messages)) or \
                (not one and any(len(bytes(k)) != 32 for k in pk)):
            raise ValueError("one 32-byte key, or one a message")
        lens = [_nbytes(m) for m in messages]
        offs, total = _layout(lens)
        src = self._pack(messages, offs, 0, total, wipe=True)
        dst = self._new(total)
        self._run_sealed(_SEAL, lens, b"", pks, src, offs, dst, offs)
        return dst, offs, lens

    # ---------------- seed dicts ----------------

    # Batches below this stay on `_core.crypto`, one box at a time. A call
    # costs about 1 ms whatever the batch (one ladder is 0.69 ms deep), the CPU
    # 41 us a seed opened and 81 us sealed: at 16 seeds the CPU opens faster
    # (0.65 against 1.12 ms), at 64 the device does (1.09 against 2.59 ms open,
    # 0.94 against 5.14 ms seal), the smallest measured size where it wins both
    # ways (scripts/box_bench.py --device-keys --seed-sweep,
    # profiles/r19_x25519_gpu.md).
    SEEDS_MIN_BATCH = 64

    def open_seeds(self, enc_seeds, pk, sk):
        """Open the 80-byte sealed seeds of a sum2 seed dict: 32-byte seeds as
        host bytes, None where the tag fails (or the entry is no 80 bytes)."""
        enc_seeds = [bytes(e) for e in enc_seeds]
        pk, sk = bytes(pk), bytes(sk)
        if len(enc_seeds) < self.SEEDS_MIN_BATCH:
            return [_crypto.sealbox_open(e, pk, sk) if len(e) == 80 else None for e in enc_seeds]
        live = [i for i, e in enumerate(enc_seeds) if len(e) == 80]
        out = [None] * len(enc_seeds)
        if not live:
            return out
        _, ok = self.sealbox_open_batch([enc_seeds[i] for i in live], pk, sk, device_keys=True)
        host = self.opened_buffer.cpu().numpy()
        for i, off, good in zip(live, self.opened_offsets, ok.tolist()):
            if good:
                out[i] = host[off:off + 32].tobytes()
        self.opened_buffer.zero_()  # plain seeds: the host copy is the one handed on
        return out

    def seal_seed(self, seed, pks):
        """Seal one 32-byte seed to every key of `pks`: 80-byte boxes as host
        bytes, in order."""
        seed, pks = bytes(seed), [bytes(k) for k in pks]
        if len(seed) != 32:
            raise ValueError("a seed is 32 bytes")
        if len(pks) < self.SEEDS_MIN_BATCH:
            return [_crypto.sealbox_seal(seed, k) for k in pks]
        dst, offs, _ = self._sealbox_seal_device([seed] * len(pks), pks)
        host = dst.cpu().numpy()
        return [host[off - 48:off + 32].tobytes() for off in offs]

    # ---------------- Ed25519 ----------------

    def _verify(self, sig_offs, pk_offs, msg_offs, msg_lens, msg_bufs, data, extra=None):
        """K10 over descriptors into `data` (and `extra`): one 0 / 1 a signature."""
        n = len(sig_offs)
        with torch.cuda.device(self.device):
            work_bytes = _hip._verify_plan(n)
            if self._work is None or self._work.numel() < work_bytes:
                self._work = self._new(work_bytes)
            ok = torch.empty(n, dtype=torch.int32, device=self.device)
            if self.time_kernels:
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
            _hip._verify_run(sig_offs, pk_offs, msg_offs, msg_lens, msg_bufs, data.data_ptr(),
                             data.numel(), 0 if extra is None else extra.data_ptr(),
                             0 if extra is None else extra.numel(), self._work.data_ptr(),
                             self._work.numel(), ok.data_ptr())
            if self.time_kernels:
                t1.record()
                t1.synchronize()
                self.kernel_ms = t0.elapsed_time(t1)
        return ok.tolist()

    def verify_batch(self, signatures, messages, pks):
        """Ed25519: whether signatures[i] is one of messages[i] under pks[i]
        (or under the one key `pks`), a list of bools. Items are host buffers
        or device tensors. Always on the device (K10), with the acceptance
        rules of `_core.crypto.verify_detached`: s >= L and keys that are no
        point are rejected, keys and R of small order are not."""
        n = len(signatures)
        one = isinstance(pks, (bytes, bytearray, memoryview, torch.Tensor))
        keys = [pks] if one else list(pks)
        if len(messages) != n or (not one and len(keys) != n) or \
                any(_nbytes(g) != 64 for g in signatures) or any(_nbytes(k) != 32 for k in keys):
            raise ValueError("one 64-byte signature and one message each, one 32-byte key or "
                             "one each")
        if n == 0:
            return []
        # key(s) | signatures | messages, every message on a 64-byte boundary
        lens = [_nbytes(m) for m in messages]
        pk_offs = [32 * i for i in range(len(keys))]
        at = (32 * len(keys) + 63) // 64 * 64
        sig_offs = [at + 64 * i for i in range(n)]
        at += 64 * n
        msg_offs = []
        for m in lens:
            msg_offs.append(at)
            at += (m + 63) // 64 * 64
        data = self._pack(keys + list(signatures) + list(messages), pk_offs + sig_offs + msg_offs,
                          0, at + _HEAD)
        ok = self._verify(sig_offs, pk_offs * n if one else pk_offs, msg_offs, lens, [0] * n, data)
        return [bool(v) for v in ok]

    def open_messages(self, sealed, pk, sk, round_seed=None):
        """Open sealed PET messages (K9, K8) and check their signatures (K10)
        where the plaintexts lie on the device. Returns (messages, flags):
        messages as `sealbox_open_batch` returns them, and an int a message.
        Bit 0: the box opened, holds a header (136 bytes) whose length field
        lies in [136, len], and the header signature over [64, length) verifies
        under the key at [64, 96). With `round_seed`, for a message of tag 1, 2
        or 3 that is no multipart chunk and long enough: bit 1, the sum
        signature at 136 verifies over round_seed || "sum"; bit 2 (tag 2), the
        update signature at 200 over round_seed || "update". A failed
        signature zeroes nothing; the eligibility threshold stays on the host."""
        return self._open_messages(sealed, pk, sk, round_seed)[:2]

    def _open_messages(self, sealed, pk, sk, round_seed):
        """open_messages, and (length, tag, flag byte) of every header whose
        length field holds, by message."""
        messages, _ = self.sealbox_open_batch(sealed, pk, sk, device_keys=True)
        flags, headers = [0] * len(messages), {}
        live = [i for i, m in enumerate(messages) if m is not None and m.numel() >= 136]
        if not live:
            return messages, flags, headers
        data = self.opened_buffer
        offs = [self.opened_offsets[i] for i in live]
        at = torch.tensor(offs, device=self.device)[:, None] + 128 + \
            torch.arange(6, device=self.device)
        heads = data[at.reshape(-1)].reshape(-1, 6).cpu().numpy()
        extra = None
        if round_seed is not None:  # the two task strings, uploaded once
            tasks = [bytes(round_seed) + b"sum", bytes(round_seed) + b"update"]
            task_offs = [0, (len(tasks[0]) + 63) // 64 * 64]
            extra = self._pack(tasks, task_offs, 0, task_offs[1] + len(tasks[1]) + _HEAD)
        jobs = []  # (message, bit, signature, message offset, length, buffer)
        for i, off, head in zip(live, offs, heads):
            length = int.from_bytes(bytes(head[:4]), "big")
            if not 136 <= length <= messages[i].numel():
                continue
            headers[i] = (length, int(head[4]), int(head[5]))
            jobs.append((i, 1, off, off + 64, length - 64, 0))
            if extra is None or head[5] & 1 or head[4] not in (1, 2, 3):
                continue
            if length >= 200:
                jobs.append((i, 2, off + 136, task_offs[0], len(tasks[0]), 1))
            if head[4] == 2 and length >= 264:
                jobs.append((i, 4, off + 200, task_offs[1], len(tasks[1]), 1))
        if jobs:
            pk_offs = [self.opened_offsets[j[0]] + 64 for j in jobs]
            ok = self._verify([j[2] for j in jobs], pk_offs, [j[3] for j in jobs],
                              [j[4] for j in jobs], [j[5] for j in jobs], data, extra)
            for (i, bit, *_), good in zip(jobs, ok):
                flags[i] |= bit * good
        return messages, flags, headers

    def open_updates(self, sealed, pk, sk, round_seed, engine, pool, row=0):
        """open_messages, then the masked vector of every update message whose
        three signatures verify (flags 7, tag 2, no multipart chunk) from the
        opened buffer into `pool` rows from `row` on (K11,
        `engine.stage_updates`): no plaintext goes to the host. Returns
        (flags, staged, index): flags as open_messages gives them, staged the
        engine's result and index[j] the message staged object j came from.
        The MaskObject starts at byte 264 of a message; the seed dict behind
        it is not parsed here."""
        _, flags, headers = self._open_messages(sealed, pk, sk, round_seed)
        index = [i for i, f in enumerate(flags)
                 if f == 7 and headers[i][1] == 2 and not headers[i][2] & 1]
        buffer = self.opened_buffer if index else self._new(0)
        staged = engine.stage_updates(buffer, [self.opened_offsets[i] + 264 for i in index],
                                      [headers[i][0] - 264 for i in index], pool, row)
        return flags, staged, index

    def open_update_sets(self, sealed, pk, sk, round_seed, engine, pool, row=0):
        """open_updates for updates that come as multipart chunks as well:
        the chunks of a batch are grouped into sets (`chunk_sets`), and the
        masked vector of every complete set is gathered from where its chunks
        lie in the opened buffer into a `pool` row (K12,
        `engine.stage_segments`). A single-part update is a set of one and
        takes the same path. Returns (flags, staged, index, pending,
        host_sets): flags as open_messages gives them, staged the engine's
        result, index[j] the messages, in chunk order, staged object j came
        from, pending the chunk messages whose set is not complete in this
        batch (nothing is kept between calls: the caller resubmits them with
        the rest, or hands them to the CPU path), and host_sets the complete
        sets whose chunk 0 is too short to hold both task signatures, which
        are not staged. A set is staged when every chunk's header signature
        verifies and has tag 2 and the sum and update signatures, at bytes 144
        and 208 of chunk 0, verify (a second K10 call). The seed dict behind
        the object is not parsed here."""
        _, flags, headers = self._open_messages(sealed, pk, sk, round_seed)
        live = [i for i, f in enumerate(flags) if f & 1 and
                (not headers[i][2] & 1 or headers[i][0] >= 144)]
        data = self.opened_buffer if live else self._new(0)
        entries = []
        if live:
            # the participant key, length | tag | flags, and the chunk header
            field = torch.tensor(list(range(64, 96)) + list(range(128, 134)) +
                                 list(range(136, 141)), device=self.device)
            at = torch.tensor([self.opened_offsets[i] for i in live],
                              device=self.device)[:, None] + field
            for i, f in zip(live, data[at.reshape(-1)].reshape(len(live), -1).cpu().numpy()):
                multi = int(f[37]) & 1
                entries.append((f[:32].tobytes(), int(f[36]), multi,
                                int.from_bytes(f[38:40].tobytes(), "big"),
                                int.from_bytes(f[40:42].tobytes(), "big"), int(f[42]) & 1,
                                headers[i][0] - (144 if multi else 136)))
        sets, host_sets, pending = chunk_sets(entries)
        sets = [s for s in sets if all(entries[e][1] == 2 for e in s)]
        off = [self.opened_offsets[i] for i in live]
        multi = [s for s in sets if entries[s[0]][2]]
        good = {id(s): flags[live[s[0]]] == 7 for s in sets if not entries[s[0]][2]}
        if multi:
            tasks = [bytes(round_seed) + b"sum", bytes(round_seed) + b"update"]
            task_offs = [0, (len(tasks[0]) + 63) // 64 * 64]
            extra = self._pack(tasks, task_offs, 0, task_offs[1] + len(tasks[1]) + _HEAD)
            heads = [off[s[0]] for s in multi for _ in range(2)]
            ok = self._verify([h + 144 + 64 * (j & 1) for j, h in enumerate(heads)],
                              [h + 64 for h in heads], task_offs * len(multi),
                              [len(tasks[0]), len(tasks[1])] * len(multi), [1] * len(heads),
                              data, extra)
            for j, s in enumerate(multi):
                good[id(s)] = bool(ok[2 * j] and ok[2 * j + 1])
        sets = [s for s in sets if good[id(s)]]
        objects = []
        for s in sets:
            if entries[s[0]][2]:
                # the chunks' data, less the two task signatures in front
                pieces = [(off[e] + 144, entries[e][6]) for e in s]
                pieces[0] = (pieces[0][0] + 128, pieces[0][1] - 128)
            else:
                pieces = [(off[s[0]] + 264, entries[s[0]][6] - 128)]
            objects.append(pieces)
        staged = engine.stage_segments(data, objects, pool, row)
        return (flags, staged, [[live[e] for e in s] for s in sets],
                [live[e] for e in pending], [[live[e] for e in s] for s in host_sets])

    # ---------------- the MAC alone ----------------

    def poly1305(self, data, key32) -> bytes:
        """Poly1305 of `data` under the one-time key through the tile and
        finish kernels; the 16-byte tag."""
        n = _nbytes(data)
        offs, total = _layout([n])
        src = self._pack([data], offs, 0, total)
        tag = self._new(16)
        self._run(_MAC, [n], [key32], [], src, offs, tag, [0])
        return bytes(tag.cpu().numpy())
