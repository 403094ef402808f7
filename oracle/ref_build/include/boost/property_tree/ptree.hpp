/* Stand-in for <boost/property_tree/ptree.hpp>: a flat "Section.key" -> text map with get<T>().  A missing key or a value that does
 * not convert as a whole throws; the reference programs catch nothing, so the program terminates, as with ptree_bad_path. */
#pragma once
#include <map>
#include <sstream>
#include <stdexcept>
#include <string>

namespace boost {
namespace property_tree {

struct ptree_error : std::runtime_error {
	explicit ptree_error(const std::string &what) : std::runtime_error(what) {}
};
struct ptree_bad_path : ptree_error {
	explicit ptree_bad_path(const std::string &what) : ptree_error(what) {}
};
struct ptree_bad_data : ptree_error {
	explicit ptree_bad_data(const std::string &what) : ptree_error(what) {}
};

struct ptree {
	std::map<std::string, std::string> values;

	template <class T>
	T get(const std::string &path) const
	{
		auto it = values.find(path);
		if (it == values.end()) throw ptree_bad_path("No such node (" + path + ")");
		return convert(it->second, path, static_cast<T *>(nullptr));
	}

private:
	static std::string convert(const std::string &text, const std::string &, std::string *) { return text; }

	template <class T>
	static T convert(const std::string &text, const std::string &path, T *)
	{
		std::istringstream in(text);
		T value;
		in >> value;
		if (!in.fail() && !in.eof()) in >> std::ws;
		if (in.fail() || !in.eof()) throw ptree_bad_data("conversion of data failed (" + path + " = " + text + ")");
		return value;
	}
};

}  // namespace property_tree
}  // namespace boost
