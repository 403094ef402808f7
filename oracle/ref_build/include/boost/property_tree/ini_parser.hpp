/* Stand-in for <boost/property_tree/ini_parser.hpp>: read_ini with the conventions crd_config_load_ini follows -- a line whose
 * first non-blank character is '#' or ';' is a comment, "[Section]", "key = value" with both sides trimmed; a line without '=',
 * an unclosed '[', an empty key and a duplicate key are errors (thrown, uncaught by the reference programs). */
#pragma once
#include <cctype>
#include <fstream>
#include <string>

#include "ptree.hpp"

namespace boost {
namespace property_tree {
namespace ini_parser {

struct ini_parser_error : ptree_error {
	explicit ini_parser_error(const std::string &what) : ptree_error(what) {}
};

inline std::string trim(const std::string &s)
{
	size_t a = 0, b = s.size();
	while (a < b && std::isspace((unsigned char)s[a])) a++;
	while (b > a && std::isspace((unsigned char)s[b - 1])) b--;
	return s.substr(a, b - a);
}

inline void read_ini(const std::string &path, ptree &pt)
{
	std::ifstream in(path.c_str());
	if (!in) throw ini_parser_error("cannot open " + path);
	std::string line, section;
	int number = 0;
	while (std::getline(in, line)) {
		number++;
		const std::string where = " at line " + std::to_string(number) + " of " + path;
		line = trim(line);
		if (line.empty() || line[0] == '#' || line[0] == ';') continue;
		if (line[0] == '[') {
			if (line[line.size() - 1] != ']') throw ini_parser_error("unmatched '['" + where);
			section = trim(line.substr(1, line.size() - 2));
			continue;
		}
		const size_t eq = line.find('=');
		if (eq == std::string::npos) throw ini_parser_error("'=' character not found" + where);
		const std::string key = trim(line.substr(0, eq));
		if (key.empty()) throw ini_parser_error("key expected" + where);
		const std::string full = section.empty() ? key : section + "." + key;
		if (pt.values.count(full)) throw ini_parser_error("duplicate key name '" + full + "'" + where);
		pt.values[full] = trim(line.substr(eq + 1));
	}
}

}  // namespace ini_parser
}  // namespace property_tree
}  // namespace boost
