"""Labelled reference clouds in the Aftr text format ("(x, y, z) <class> <part>" per line), the input of the semantic ICP
(ops.icp_reference / ops.semantic_icp)."""
import ctypes as C

import numpy as np


def read_labelled_cloud(path: str, part_labels, class_labels=None):
    """One Aftr frame -> (xyz (n, 3) float32, part ids (n,) int32 in ``part_labels`` order), through the native frame parser
    of PointCloudSet (the reference's per-line rules; rows with a non-finite coordinate are dropped).  ``class_labels``
    defaults to the class names the file itself uses.  An unknown part label raises, like PointCloudSet."""
    from .PointCloudSet import _hostlib
    with open(path, "rb") as f:
        text = f.read()
    if class_labels is None:
        class_labels = []
        for line in text.decode(errors="replace").splitlines():
            toks = [t for t in line[line.find(")") + 1:].split(" ") if len(t) > 1] if ")" in line else []
            if toks and toks[0] not in class_labels:
                class_labels.append(toks[0])
    part_labels = list(part_labels)
    h = _hostlib()
    max_pts = text.count(b"\n") + 1
    xyz = np.empty((max_pts, 3), dtype=np.float64)
    part = np.empty(max_pts, dtype=np.int32)
    cn = (C.c_char_p * max(len(class_labels), 1))(*[k.encode() for k in class_labels])
    pn = (C.c_char_p * max(len(part_labels), 1))(*[k.encode() for k in part_labels])
    cls, nonf, errl = C.c_int32(), C.c_long(), C.c_long()
    n = h.pn_parse_aftr_frame(text, len(text), cn, len(class_labels), pn, len(part_labels), xyz.ctypes.data, part.ctypes.data,
                              max_pts, C.byref(cls), C.byref(nonf), C.byref(errl))
    if n < 0:
        line = text.split(b"\n")[errl.value].decode(errors="replace").strip()
        kind = {-2: "unknown class label", -3: "unknown part label"}.get(n, "malformed line")
        raise ValueError(f"{path}: {kind} on line {errl.value}: {line!r}")
    return xyz[:n].astype(np.float32), part[:n].copy()
