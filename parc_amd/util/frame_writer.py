"""Frame sink of the headless viewer: device image -> pinned host copy -> bounded queue -> one writer thread that encodes PNG.

The caller's loop never waits on encoding: ``submit`` enqueues an asynchronous device-to-host copy and returns; when every pinned
buffer is still in flight the frame is dropped and counted (printed by ``close``, which also runs at interpreter exit).  The PNG
encoder uses the standard library only (zlib + struct).
"""
from __future__ import annotations

import atexit
import os
import queue
import struct
import threading
import zlib

import numpy as np


def encode_png(img: np.ndarray, level: int = 3) -> bytes:
    """PNG bytes of an ``uint8 [H, W, 4]`` (RGBA) or ``[H, W, 3]`` (RGB) array: 8-bit, no interlace, filter 0 on every row."""
    img = np.ascontiguousarray(img, np.uint8)
    if img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError("encode_png: expected [H, W, 3|4] uint8")
    h, w, c = img.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * c)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    ihdr = struct.pack(">IIBBBBB", w, h, 8, 6 if c == 4 else 2, 0, 0, 0)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", ihdr) + chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b"")


class FrameWriter:
    """Writes ``pattern % index`` PNG files into ``out_dir``; ``index`` counts submitted frames (a dropped frame leaves a gap)."""

    def __init__(self, out_dir, queue_size=8, pattern="frame_%06d.png"):
        self.out_dir = out_dir
        self.pattern = pattern
        self.submitted = 0
        self.written = 0
        self.dropped = 0
        self._queue_size = max(int(queue_size), 1)
        self._free = None          # pinned host buffers not in flight (created on the first frame, shape fixed from then on)
        self._q = queue.Queue(maxsize=self._queue_size)
        self._thread = None
        self._closed = False
        self._error = None
        os.makedirs(out_dir, exist_ok=True)
        atexit.register(self.close)

    def submit(self, frame_dev) -> bool:
        """Queue one ``uint8 [H, W, 4]`` device image; returns False when it was dropped (every buffer in flight)."""
        import torch
        if self._closed:
            raise RuntimeError("FrameWriter is closed")
        if self._error is not None:
            raise RuntimeError(f"frame writer thread failed: {self._error}")
        idx = self.submitted
        self.submitted += 1
        if self._free is None:
            self._free = queue.Queue()
            for _ in range(self._queue_size):
                self._free.put(torch.empty(tuple(frame_dev.shape), dtype=torch.uint8, pin_memory=True))
            self._thread = threading.Thread(target=self._run, name="parc-frame-writer", daemon=True)
            self._thread.start()
        try:
            buf = self._free.get_nowait()
        except queue.Empty:
            self.dropped += 1
            return False
        buf.copy_(frame_dev, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(frame_dev.device))
        self._q.put_nowait((idx, buf, ev))  # never blocks: at most queue_size buffers exist
        return True

    def _run(self):
        while True:
            item = self._q.get()
            if item is None:
                return
            idx, buf, ev = item
            try:
                ev.synchronize()
                data = encode_png(buf.numpy())
                with open(os.path.join(self.out_dir, self.pattern % idx), "wb") as f:
                    f.write(data)
                self.written += 1
            except Exception as ex:  # noqa: BLE001  reported by the next submit / close
                self._error = ex
            finally:
                self._free.put(buf)

    def close(self):
        """Finish the queued frames, stop the thread and print the count of dropped frames."""
        if self._closed:
            return
        self._closed = True
        if self._thread is not None:
            self._q.put(None)
            self._thread.join()
        print("frame writer: %d frame(s) written to %s, %d dropped (queue full)" % (self.written, self.out_dir, self.dropped))
        if self._error is not None:
            raise RuntimeError(f"frame writer thread failed: {self._error}")
