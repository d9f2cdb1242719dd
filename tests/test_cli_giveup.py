"""fba_experiment ... --on-giveup / --reject-attempts / --retired-file: the usage text and the refusals that need no device."""
import subprocess

import pytest

import fba_pomdp_amd as fba


@pytest.fixture(scope="module")
def cli():
    fba.build()
    return fba.build_cli()


def test_the_usage_names_the_flags(cli):
    r = subprocess.run([cli, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    text = r.stdout + r.stderr
    assert "--on-giveup stop|retire" in text and "(fba_giveup_policy)" in text
    assert "--reject-attempts N" in text and "a multiple of 1024" in text
    assert "--retired-file FILE" in text and "run episode t slot reason counted max_attempts" in text


def test_bad_arguments_are_refused(cli, tmp_path):
    base = [cli, "bapomdp", "-D", "episodic-tiger", "-f", str(tmp_path / "x.res")]
    r = subprocess.run(base + ["--on-giveup", "ignore"], capture_output=True, text=True)
    assert r.returncode == 1 and "the argument ('ignore') for option '--on-giveup' is invalid" in r.stderr
    r = subprocess.run(base + ["--reject-attempts", "many"], capture_output=True, text=True)
    assert r.returncode == 1 and "the argument ('many') for option '--reject-attempts' is invalid" in r.stderr
    assert not (tmp_path / "x.res").exists()
