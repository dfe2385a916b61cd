"""Every public header, alone and through include/gcnk.h, is C99 and C++17 to the host compilers: each family header
is self-contained (its own guard, <stdint.h> and extern "C"), so a caller may include one without the rest.  Syntax
only, no GPU and no library; skipped where there is no host compiler."""
import os
import shutil
import subprocess

import pytest

import gcn_amd  # noqa: F401
from graph_convolutional_networks_for_text_classification_amd import _lib

LANGUAGES = {"c": ("cc", ["-x", "c", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-fsyntax-only"]),
             "c++": ("c++", ["-x", "c++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only"])}


@pytest.mark.parametrize("language", LANGUAGES)
def test_each_public_header_compiles_alone(language, tmp_path):
    compiler, flags = LANGUAGES[language]
    if shutil.which(compiler) is None:
        pytest.skip(f"no {compiler} on the path")
    assert len(_lib.HEADERS) == 4
    for path in _lib.HEADERS:
        source = tmp_path / ("only_" + os.path.basename(path) + (".c" if language == "c" else ".cpp"))
        # twice: the guard holds; a use of int32_t: the header brought <stdint.h> itself
        source.write_text(f'#include "{os.path.basename(path)}"\n#include "{os.path.basename(path)}"\n'
                          "int32_t only_this_header = 0;\n")
        run = subprocess.run([compiler, *flags, "-I", os.path.dirname(path), str(source)], capture_output=True,
                             text=True)
        assert run.returncode == 0, f"{os.path.basename(path)} as {language}:\n{run.stderr}"
