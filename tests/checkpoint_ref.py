"""A reader and a writer of the checkpoint format, version 1, written from the
text of DESIGN.md 3.16 in numpy.  It does not import the library: the tests
hold the library's files against it and feed the library its files.

    write(path, config, sections, flags=None)   sections: {tag: bytes / ndarray}
    read(path) -> dict                          header, directory, arrays, texts
    checksum(data) -> int
"""
import struct

import numpy as np

MAGIC = b"FRECSYS1"
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
# CONFIG's numeric fields in file order: (name, is_float)
CONFIG_FIELDS = (("dim", 0), ("l2_reg", 1), ("l2_reg_exp", 1), ("uobs_weight", 1), ("stdev", 1),
                 ("alpha", 1), ("bandwidth", 1), ("stepsize", 1), ("sampling_ratio", 1),
                 ("block_size", 0), ("xi_iterations", 0), ("pd_iterations", 0),
                 ("use_epanechnikov", 0), ("use_snr", 0), ("print_train_stats", 0),
                 ("print_residual_stats", 0), ("print_var_stats", 0), ("seed", 0),
                 ("parity_quirks", 0), ("use_cg", 0), ("cg_error_tolerance", 1),
                 ("cg_max_iterations", 0))
CONFIG_DEFAULTS = dict(dim=8, l2_reg=0.002, l2_reg_exp=1.0, uobs_weight=0.1, stdev=0.1, alpha=0.3,
                       bandwidth=1.0, stepsize=0.1, sampling_ratio=0.1, block_size=64,
                       xi_iterations=5, pd_iterations=1, use_epanechnikov=0, use_snr=0,
                       print_train_stats=1, print_residual_stats=0, print_var_stats=0, seed=-1,
                       parity_quirks=1, use_cg=0, cg_error_tolerance=1e-10, cg_max_iterations=100)
COUNTS = ("n_users", "n_items", "n_tuples", "epochs_trained", "tuples_checksum")
DUAL_MODELS = ("safer2", "safer2pp", "erm_mf", "cvar_mf")


def _raw(data) -> bytes:
    if isinstance(data, (bytes, bytearray)):
        return bytes(data)
    if isinstance(data, str):
        return data.encode()
    return np.ascontiguousarray(data).tobytes()


def checksum(data) -> int:
    """sum_i mix(w_i + (i + 1) * golden) mod 2^64 over the zero-padded u64 words."""
    raw = _raw(data)
    w = np.frombuffer(raw + b"\0" * (-len(raw) % 8), dtype="<u8")
    with np.errstate(over="ignore"):
        z = w + np.arange(1, len(w) + 1, dtype=np.uint64) * GOLDEN
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return int((z ^ (z >> np.uint64(31))).sum(dtype=np.uint64))


def tuples_checksum(users, items) -> int:
    return checksum(_raw(np.asarray(users, dtype="<i4")) + _raw(np.asarray(items, dtype="<i4")))


def format_config(config: dict) -> str:
    """CONFIG's text; `config` holds the model flags, model_name and COUNTS."""
    full = dict(CONFIG_DEFAULTS)
    full.update(config)
    lines = []
    for name, is_float in CONFIG_FIELDS:
        v = full[name]
        lines.append(f"{name}={'%.9g' % float(np.float32(v)) if is_float else int(v)}")
    lines.append(f"model_name={full['model_name']}")
    for name in COUNTS:
        lines.append(f"{name}={int(full[name])}")
    return "".join(l + "\n" for l in lines)


def parse_lines(text: str) -> dict:
    out = {}
    for line in text.split("\n"):
        if line:
            name, value = line.split("=", 1)
            out[name] = value
    return out


def parse_config(text: str) -> dict:
    kv = parse_lines(text)
    cfg = {"model_name": kv["model_name"]}
    for name, is_float in CONFIG_FIELDS:
        cfg[name] = float(np.float32(kv[name])) if is_float else int(kv[name])
    for name in COUNTS:
        cfg[name] = int(kv[name])
    return cfg


def layout(sizes, first):
    """Offsets of sections of these sizes laid out in order from `first`."""
    offs, pos = [], first
    for n in sizes:
        pos = (pos + 63) // 64 * 64
        offs.append(pos)
        pos += n
    return offs, pos


def pack(sections, flags, version=1):
    """The bytes of a file holding `sections` ([(tag, bytes)]) in this order."""
    raws = [(t, _raw(d)) for t, d in sections]
    offs, total = layout([len(r) for _, r in raws], 64 + 32 * len(raws))
    directory = b"".join(struct.pack("<8sQQQ", t.encode(), o, len(r), checksum(r))
                         for (t, r), o in zip(raws, offs))
    head = struct.pack("<8sIIQQQ24s", MAGIC, version, len(raws), total, flags, checksum(directory),
                       b"")
    out = bytearray(total)
    out[:64] = head
    out[64:64 + len(directory)] = directory
    for (t, r), o in zip(raws, offs):
        out[o:o + len(r)] = r
    return bytes(out)


def model_sections(config, U, V, loss, omega=None, item_reg=None, users=None, items=None,
                   state=""):
    """[(tag, data)] of one model, CONFIG's counts filled in from the arrays."""
    U = np.ascontiguousarray(U, dtype="<f4")
    V = np.ascontiguousarray(V, dtype="<f4")
    cfg = dict(config)
    cfg.update(dim=U.shape[1], n_users=U.shape[0], n_items=V.shape[0])
    cfg.setdefault("epochs_trained", 0)
    secs = []
    if users is not None:
        users = np.ascontiguousarray(users, dtype="<i4")
        items = np.ascontiguousarray(items, dtype="<i4")
        cfg["n_tuples"] = len(users)
        cfg["tuples_checksum"] = tuples_checksum(users, items)
        secs += [("USERS", users), ("ITEMS", items)]
    secs += [("LOSS", np.ascontiguousarray(loss, dtype="<f4"))]
    if omega is not None:
        secs += [("OMEGA", np.ascontiguousarray(omega, dtype="<f4")),
                 ("ITEMREG", np.ascontiguousarray(item_reg, dtype="<f4"))]
    secs += [("U", U), ("V", V)]
    return [("CONFIG", format_config(cfg)), ("STATE", state)] + secs


def write(path, sections, flags=None):
    if flags is None:
        flags = int(any(t == "USERS" for t, _ in sections))
    with open(path, "wb") as f:
        f.write(pack(sections, flags))


def read(path) -> dict:
    """Everything of a file, every rule of the format asserted on the way."""
    raw = open(path, "rb").read()
    assert len(raw) >= 64 and raw[:8] == MAGIC
    version, n, total, flags, dsum = struct.unpack_from("<IIQQQ", raw, 8)
    assert version == 1 and total == len(raw) and raw[40:64] == b"\0" * 24
    assert flags in (0, 1)
    directory = raw[64:64 + 32 * n]
    assert checksum(directory) == dsum
    out = {"version": version, "flags": flags, "total": total, "sections": {}, "raw": {}}
    covered = np.zeros(len(raw), dtype=bool)
    covered[:64 + 32 * n] = True
    for i in range(n):
        tag, off, size, csum = struct.unpack_from("<8sQQQ", directory, 32 * i)
        tag = tag.rstrip(b"\0").decode()
        assert off % 64 == 0 and off >= 64 + 32 * n and off + size <= len(raw), tag
        assert not covered[off:off + size].any(), f"{tag} overlaps"
        covered[off:off + size] = True
        assert checksum(raw[off:off + size]) == csum, f"{tag}: checksum"
        out["sections"][tag] = (off, size, csum)
        out["raw"][tag] = raw[off:off + size]
    gaps = np.frombuffer(raw, dtype=np.uint8)[~covered]
    assert not gaps.any(), "a gap byte is not zero"
    assert covered[-1], "bytes after the last section"
    cfg = out["config"] = parse_config(out["raw"]["CONFIG"].decode())
    out["state"] = parse_lines(out["raw"]["STATE"].decode())
    nu, ni, d = cfg["n_users"], cfg["n_items"], cfg["dim"]
    f4 = lambda t, *shape: np.frombuffer(out["raw"][t], dtype="<f4").reshape(shape)
    out["U"], out["V"], out["loss"] = f4("U", nu, d), f4("V", ni, d), f4("LOSS", nu)
    dual = cfg["model_name"] in DUAL_MODELS
    assert ("OMEGA" in out["raw"]) == dual and ("ITEMREG" in out["raw"]) == dual
    if dual:
        out["omega"], out["item_reg"] = f4("OMEGA", nu), f4("ITEMREG", ni)
    assert ("USERS" in out["raw"]) == bool(flags & 1) == ("ITEMS" in out["raw"])
    if flags & 1:
        out["users"] = np.frombuffer(out["raw"]["USERS"], dtype="<i4")
        out["items"] = np.frombuffer(out["raw"]["ITEMS"], dtype="<i4")
        assert len(out["users"]) == cfg["n_tuples"] == len(out["items"])
        assert tuples_checksum(out["users"], out["items"]) == cfg["tuples_checksum"]
    return out
