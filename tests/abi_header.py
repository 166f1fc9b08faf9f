"""What include/mtr.h declares, read from its text: the one parser the ABI tests share."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "mtr.h")
_PROTO = r"\b(mtr_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;"


def _text(hdr=HDR):
    return re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)


def declared(hdr=HDR):
    """the sorted names of the functions a header declares"""
    return sorted(set(re.findall(r"\b(mtr_[a-z0-9_]+)\s*\(", _text(hdr))))


def prototypes():
    """name -> argument count of every prototype of include/mtr.h"""
    return {m.group(1): len([a for a in m.group(2).split(",") if a.strip() and a.strip() != "void"])
            for m in re.finditer(_PROTO, _text())}


def return_types():
    """name -> declared return type of every prototype of include/mtr.h, as one normalised string ('const char *')"""
    out = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \t\n]*?[ \t\n*]+)" + _PROTO, _text()):
        words = [w for w in re.sub(r"\*", " * ", m.group(1)).split() if w not in ("MTR_API", "extern")]
        out[m.group(2)] = " ".join(words)
    return out
