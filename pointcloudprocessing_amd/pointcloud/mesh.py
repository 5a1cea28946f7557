"""A labelled triangle mesh from a Wavefront OBJ with one named sub-mesh per part: what the reference's SemanticMeshICP tab
loads.  A small reader in pure Python/NumPy: geometry and the o / g names only; and the writer that puts a mesh made by
ops.reconstruct_mesh / ops.scans_to_mesh into the same form."""
from __future__ import annotations

import numpy as np

_SKIPPED = ("vn", "vt", "vp", "usemtl", "mtllib", "s", "l", "p")


def read_labelled_mesh(path: str, part_labels, name_map=None):
    """One OBJ file -> (vertices (V, 3) float32, faces (F, 3) int32 into ``vertices``, part ids (F,) int32 in ``part_labels``
    order).  Read: ``v x y z`` (further columns ignored); ``f`` with corners ``i``, ``i/t``, ``i//n`` or ``i/t/n`` (only the
    vertex index is used), 1-based or negative (relative to the vertices read so far), polygons fan-triangulated from their
    first corner.  The part of a face is the current ``g`` name, or the current ``o`` name when no ``g`` has been set since it;
    the name is looked up in ``part_labels``, through ``name_map`` (name -> part label) when it has the name.  A face under an
    unknown name, or before any name, raises ValueError with the line number (counted from 0), like read_labelled_cloud for an unknown part.
    ``vn``, ``vt``, ``usemtl``, ``mtllib``, ``s`` and comments are skipped."""
    part_labels = list(part_labels)
    name_map = dict(name_map or {})
    verts, faces, parts = [], [], []
    o_name = g_name = None
    with open(path, "r", errors="replace") as f:
        for ln, raw in enumerate(f):
            line = raw.split("#", 1)[0].strip()
            if not line:
                continue
            toks = line.split()
            key, args = toks[0], toks[1:]
            if key == "v":
                if len(args) < 3:
                    raise ValueError(f"{path}: malformed vertex on line {ln}: {raw.strip()!r}")
                try:
                    verts.append([float(args[0]), float(args[1]), float(args[2])])
                except ValueError:
                    raise ValueError(f"{path}: malformed vertex on line {ln}: {raw.strip()!r}") from None
            elif key == "o":
                o_name, g_name = " ".join(args) or None, None
            elif key == "g":
                g_name = " ".join(args) or None
            elif key == "f":
                name = g_name if g_name is not None else o_name
                label = name_map.get(name, name)
                if label not in part_labels:
                    raise ValueError(f"{path}: unknown part label on line {ln}: {name!r}")
                if len(args) < 3:
                    raise ValueError(f"{path}: a face needs three corners, line {ln}: {raw.strip()!r}")
                corners = []
                for a in args:
                    try:
                        i = int(a.split("/", 1)[0])
                    except ValueError:
                        raise ValueError(f"{path}: malformed face on line {ln}: {raw.strip()!r}") from None
                    i = i - 1 if i > 0 else len(verts) + i
                    if i < 0 or i >= len(verts) or a.startswith("0"):
                        raise ValueError(f"{path}: vertex index out of range on line {ln}: {raw.strip()!r}")
                    corners.append(i)
                for k in range(1, len(corners) - 1):
                    faces.append([corners[0], corners[k], corners[k + 1]])
                    parts.append(part_labels.index(label))
            elif key in _SKIPPED:
                continue
            # anything else (curves, surfaces, extensions) carries no triangles: ignored
    return (np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(faces, np.int32).reshape(-1, 3),
            np.asarray(parts, np.int32).reshape(-1))


def write_labelled_mesh(path: str, vertices, faces, face_labels, part_names) -> None:
    """(vertices (V, 3), faces (F, 3) into them, face_labels (F,) in [0, len(part_names)), part_names) -> one OBJ file with one named
    sub-mesh (``g name``) per part, which ``read_labelled_mesh(path, part_names)`` reads back to the same faces in the same order,
    the same labels and the same fp32 vertices (nine significant digits round-trip an fp32 value).  The faces keep their order: a
    ``g`` line stands wherever the label changes, and a repeated ``g name`` continues that part's sub-mesh.  Arrays or tensors."""
    v = np.asarray(vertices.cpu() if hasattr(vertices, "cpu") else vertices, np.float32).reshape(-1, 3)
    f = np.asarray(faces.cpu() if hasattr(faces, "cpu") else faces, np.int64).reshape(-1, 3)
    lab = np.asarray(face_labels.cpu() if hasattr(face_labels, "cpu") else face_labels, np.int64).reshape(-1)
    names = [str(n) for n in part_names]
    if lab.shape[0] != f.shape[0]:
        raise ValueError(f"write_labelled_mesh: {f.shape[0]} faces but {lab.shape[0]} labels")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError("write_labelled_mesh: a face refers to a vertex that does not exist")
    if lab.size and (lab.min() < 0 or lab.max() >= len(names)):
        raise ValueError(f"write_labelled_mesh: a face label lies outside [0, {len(names)})")
    if any(not n or n != " ".join(n.split()) or "#" in n for n in names) or len(set(names)) != len(names):
        raise ValueError("write_labelled_mesh: part names must be distinct, non-empty, without '#' and with single inner spaces")
    with open(path, "w") as out:
        out.write("".join(f"v {x:.9g} {y:.9g} {z:.9g}\n" for x, y, z in v.tolist()))
        last = -1
        for (a, b, c), l in zip((f + 1).tolist(), lab.tolist()):
            if l != last:
                out.write(f"g {names[l]}\n")
                last = l
            out.write(f"f {a} {b} {c}\n")
