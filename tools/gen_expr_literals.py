"""Writes tests/golden/expr_literals.bin: the ScalarValue.ipc_bytes literals
that tools/expr_fuzz.cpp draws from (it cannot encode Arrow IPC itself).

Record layout, little endian: u8 type (0 Int32, 1 Int64, 2 Float64, 3 Bool,
4 Utf8), u8 is_null, u32 length, then `length` bytes of Arrow IPC stream.
"""
import os
import struct
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

import pyarrow as pa  # noqa: E402

from blaze_amd import plan  # noqa: E402

LITERALS = [
    (0, pa.int32(), [0, 1, -1, 7, -10, 2**31 - 1, -2**31, None]),
    (1, pa.int64(), [0, 1, -1, 10, -3, 2**63 - 1, -2**63, 2**31, None]),
    (2, pa.float64(), [0.0, 1.5, -2.25, 1e30, -1e30, float("nan"), None]),
    (3, pa.bool_(), [True, False, None]),
    (4, pa.utf8(), ["x"]),
]


def main():
    out = bytearray()
    for tag, ty, values in LITERALS:
        for v in values:
            blob = plan.literal_ipc(v, ty)
            out += struct.pack("<BBI", tag, 1 if v is None else 0, len(blob))
            out += blob
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "tests", "golden", "expr_literals.bin")
    with open(path, "wb") as f:
        f.write(bytes(out))
    print(f"{path}: {len(out)} bytes")


if __name__ == "__main__":
    main()
