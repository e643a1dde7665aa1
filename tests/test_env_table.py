"""INTEGRATION.md's environment table and the sources agree on what is read."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "pacmann_amd"
SOURCES = sorted((PKG / "csrc").iterdir()) + sorted(PKG.glob("*.py"))
READ = re.compile(r'(?:getenv|env_int|environ\.get)\(\s*"(PM_[A-Z0-9_]+)"')
DEFINE = re.compile(r"^\s*#\s*define\s+(PM_[A-Z0-9_]+)", re.M)
NAME = re.compile(r"PM_[A-Z0-9_]+")


def _section() -> str:
    text = (ROOT / "INTEGRATION.md").read_text()
    start = text.index("## Environment variables")
    end = text.find("\n## ", start + 1)
    return text[start:end if end > 0 else len(text)]


def _read_names() -> set:
    return {n for p in SOURCES for n in READ.findall(p.read_text())}


def test_every_variable_read_is_documented():
    documented = set(NAME.findall(_section()))
    assert sorted(_read_names() - documented) == []


def test_every_documented_variable_exists():
    rows = [l for l in _section().splitlines() if l.startswith("| `PM_")]
    assert rows, "the environment table was not found"
    first_column = {n for l in rows for n in NAME.findall(l.split("|")[1])}
    defined = {n for p in (PKG / "csrc").iterdir() for n in DEFINE.findall(p.read_text())}
    assert sorted(first_column - _read_names() - defined) == []
